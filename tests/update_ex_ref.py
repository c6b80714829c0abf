"""rau_update_ex stated in fp64 numpy: tests/update_ref.py's noise, clip and rules, plus segments, the frozen
exclusion, decoupled weight decay and the weight average.

A segment is the weight or the bias part of one layer of a group.  `segs` below is {group: [Seg]} in layout order,
the last one ending at the group's length."""
from dataclasses import dataclass

import numpy as np

from tests import update_ref

GROUPS = update_ref.GROUPS


@dataclass
class Seg:
    end: int                # end offset in the group (exclusive)
    lr_scale: float = 1.0   # 0 freezes
    decay: float = 1.0      # the multiplier of weight_decay that applies to this segment (weight: 1, bias: 0)


def segments(layout, opts=None):
    """layout: RAU.layout(group) entries (name, offset, rows, cols), weight then bias per layer; opts: {layer index:
    (lr_scale, decay_weight, decay_bias)}, defaults (1, 1, 0).  -> [Seg]."""
    out = []
    for li, (_, off, rows, cols) in enumerate(layout):
        lr_scale, dw, db = (opts or {}).get(li // 2, (1.0, 1.0, 0.0))
        out.append(Seg(off + rows * cols, lr_scale, db if li & 1 else dw))
    return out


def per_element(segs, n):
    """-> (lr_scale[n], decay[n], frozen[n]) of a group's elements."""
    scale, decay = np.empty(n), np.empty(n)
    start = 0
    for s in segs:
        scale[start:s.end] = s.lr_scale
        decay[start:s.end] = s.decay
        start = s.end
    assert start == n
    return scale, decay, scale == 0.0


def update(x, g, m, v, ema, t, step_t, segs, noise=None, rule="adam", clip_scope="group", lr=3e-3, mult_lr=3e-4,
           b1=0.9, b2=0.999, eps=1e-8, eta=0.01, gamma=0.55, clip=0.1, weight_decay=0.0, ema_decay=0.0):
    """One rau_update_ex.  x, g, m, v, ema, noise: {group: fp64 vector} (ema may be None when ema_decay == 0);
    t: {group: update count AFTER this update}.  -> (x, g_out, m, v, ema, norms[4]).  Frozen elements keep x, g, m,
    v and ema, get no noise, and are in no norm; the decay multiplies x before the rule's step (AdamW's order) and
    enters neither the gradient nor the moments; the average follows the rule, on the new x."""
    elem = {"adam": update_ref.adam_elem, "adamax": update_ref.adamax_elem}[rule]
    coef = {k: per_element(segs[k], len(x[k])) for k in GROUPS}
    gn = {}
    for k in GROUPS:
        gk = np.array(g[k], np.float64)
        live = ~coef[k][2]
        if noise is not None and eta > 0:
            gk[live] += noise[k][live] * np.sqrt(eta / ((step_t + 1) * gamma))
        gn[k] = gk
    sq = [float(np.sum(gn[k][~coef[k][2]] ** 2)) for k in GROUPS]
    norms = [np.sqrt(s) for s in sq] + [np.sqrt(sq[0] + sq[1] + sq[2])]
    xo, go, mo, vo, eo = {}, {}, {}, {}, {}
    for i, k in enumerate(GROUPS):
        scale, decay, frozen = coef[k]
        live = ~frozen
        glr = mult_lr if k == "mult" else lr
        sc = update_ref.clip_scale(norms[3] if clip_scope == "global" else norms[i], clip)
        x0, m0, v0 = (np.asarray(a[k], np.float64) for a in (x, m, v))
        gc = gn[k] * sc
        xd = x0 * (1.0 - glr * scale * weight_decay * decay)
        xn, mn, vn = elem(xd, gc, m0, v0, t[k], glr * scale, b1, b2, eps)
        xo[k], mo[k], vo[k], go[k] = (np.where(live, new, old) for new, old in
                                      ((xn, x0), (mn, m0), (vn, v0), (gc, np.asarray(g[k], np.float64))))
        if ema is not None:
            e0 = np.asarray(ema[k], np.float64)
            eo[k] = np.where(live, ema_decay * e0 + (1.0 - ema_decay) * xo[k], e0) if ema_decay > 0 else e0
    return xo, go, mo, vo, (eo if ema is not None else None), np.array(norms)
