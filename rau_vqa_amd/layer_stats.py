"""The numpy statement of rau_layer_stats (include/rau.h, csrc/layer_stats.hip), and the accuracy bar of its sums.

The readout of one flat vector over a layout: per entry the sum of squares of the FINITE elements (in float64, the
yardstick the device's f32 sum is held to), the largest finite magnitude, and the count of NaN and +-Inf elements.
The direction is the rule's step without its step size, formed per element in float32 with one rounding per operation,
as the device forms it: Adam m / (sqrt(v) + eps), Adamax m / u.

CHUNK restates kStatChunk (csrc/kernels.h).  chain_length(n) is L(n), the length of the longest chain of additions
behind the device's sumsq of an entry of n elements, as layer_stats.hip's header derives it; bar(n) is the relative
error that chain allows against an exact sum of non-negative terms."""
from __future__ import annotations

import numpy as np

CHUNK = 8192          # kStatChunk
THREADS = 256         # threads of a workgroup of the first pass
TREE = 8              # wave_sum's 6 levels, then (w0 + w1) + (w2 + w3)

ADAM, ADAMAX = "adam", "adamax"


def chain_length(n: int) -> int:
    """L(n) = 4 ceil(floor(c / 4) / 256) + 2 + 8 + ceil(n / CHUNK), c = min(n, CHUNK): the serial additions of one
    thread (its quads, a head and a tail element), the workgroup tree, the items of the entry."""
    n = int(n)
    if n < 1:
        raise ValueError(f"chain_length: n = {n}")
    c = min(n, CHUNK)
    quads = c // 4
    serial = 4 * -(-quads // THREADS) + 2
    return serial + TREE + -(-n // CHUNK)


def bar(n: int) -> float:
    """Largest relative error of the device's f32 sum of n squares against the exact sum: L(n) rounded additions,
    the rounded square, and one more unit for the second-order terms."""
    return (chain_length(n) + 2) * 2.0 ** -24


def items_of(off: int, n: int):
    """[(start, length)]: the work items of an entry of n elements at offset off."""
    return [(s, min(CHUNK, off + n - s)) for s in range(off, off + n, CHUNK)]


def longest_chain(off: int, n: int) -> int:
    """The longest chain of additions of the order layer_stats.hip states, counted link by link for an entry at
    offset off: what chain_length bounds for every alignment."""
    worst = 0
    for s, ln in items_of(off, n):
        e = s + ln
        a0 = min((s + 3) & ~3, e)
        a1 = max(e & ~3, a0)
        head, tail, quads = a0 - s, e - a1, (a1 - a0) // 4
        per_thread = [(1 if t < head else 0) + 4 * len(range(t, quads, THREADS)) + (1 if t < tail else 0)
                      for t in range(min(THREADS, max(head, tail, quads, 1)))]
        worst = max(worst, max(per_thread))
    return worst + TREE + len(items_of(off, n))


def entry_ranges(layout, total):
    """[(name, start, end)] from a layout listing [(name, offset, rows, cols)] of a flat vector of `total` elements:
    an entry ends where the next one starts."""
    offs = [e[1] for e in layout] + [int(total)]
    return [(e[0], offs[i], offs[i + 1]) for i, e in enumerate(layout)]


def vector_stats(vec, layout):
    """[{name, n, sumsq (float64), absmax (float32), nonfinite}] of one flat vector, entry by entry."""
    vec = np.asarray(vec, np.float32).ravel()
    out = []
    for name, a, b in entry_ranges(layout, vec.size):
        x = vec[a:b]
        fin = np.isfinite(x)
        xf = x[fin].astype(np.float64)
        out.append({"name": name, "n": int(b - a), "sumsq": float(np.sum(xf * xf)),
                    "absmax": np.float32(np.max(np.abs(x[fin]))) if fin.any() else np.float32(0.0),
                    "nonfinite": int((~fin).sum())})
    return out


def direction(m, v, rule, eps):
    """The rule's direction in float32, one rounding per operation: m / (sqrt(v) + eps) or m / u (v holds u)."""
    m, v = np.asarray(m, np.float32), np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        if rule == ADAM:
            return m / (np.sqrt(v) + np.float32(eps))
        if rule == ADAMAX:
            return m / v
    raise ValueError(f"direction: rule {rule!r}")


def stats(layouts, grads=None, params=None, moments=None, rule=ADAM, eps=1e-8):
    """The whole readout.  layouts: {group: layout listing}; grads, params: {group: vector} or None; moments:
    {group: (m, v)} or None.  -> a list in layout order, group by group, of dicts with name, group, n and per source
    given ("grad", "param", "dir") a dict of sumsq, absmax and nonfinite."""
    out = []
    for g in ("embed", "rnn", "mult"):
        rows = [{"name": e[0], "group": g} for e in layouts[g]]
        for key, vec in (("grad", grads), ("param", params),
                         ("dir", None if moments is None else
                          {k: direction(mv[0], mv[1], rule, eps) for k, mv in moments.items()})):
            if vec is None:
                continue
            for row, st in zip(rows, vector_stats(vec[g], layouts[g])):
                row["n"] = st["n"]
                row[key] = {k: st[k] for k in ("sumsq", "absmax", "nonfinite")}
        out += rows
    return out
