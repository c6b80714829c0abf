"""tests/test_gpu_rows.py's CASES table held to the launch rules, without a device.

Split counts, chunk schedules, hop groups and head launches have no profile class of their own (one wgrad_gemm launch
is one launch at any split), so most of what the table says a row reaches cannot be asserted where it runs.  Here
each rule is restated in a few lines (from the file named beside it), every row's stated classes are compared with
what the restatement gives, and the coverage the table claims -- each predicate on both sides, each named edge on
both sides -- is asserted, so that a row taken out of the table fails here.
"""
import pytest

from tests.test_gpu_rows import CASES, MODULE_B, MODULE_DIMS, SEQUENCE, active, dims_of, row_id


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------- the rules, restated
def tiles128(problems):                                # 128 x 128 output tiles of (out, in) problems
    return sum(cdiv(m, 128) * cdiv(n, 128) for m, n in problems)


def mult_problems(d):                                  # rau_ctx.hip mult_wgrad_problems: the nine Linears, (out, in)
    Q = 4 * d["Rq"]
    return [(d["K"], d["M"]), (d["M"], d["R"]), (4 * d["R"], d["M"]), (4 * d["R"], d["R"]), (d["M"], d["S"]),
            (d["S"], d["R"]), (d["A"], d["M"]), (d["M"], Q), (d["M"], d["R"])]


def enc_problems(d):                                   # rau_ctx.hip enc_wgrad_problems: i2h / h2h of both layers
    return [(4 * d["Rq"], d["E"])] + [(4 * d["Rq"], d["Rq"])] * 3


def split_class(s, rows):
    """(splits, K-steps per split, K-steps of the last split, rows of the last K-step) of a request for s splits"""
    nk = cdiv(rows, 32)
    per = cdiv(nk, s)
    n = cdiv(nk, per)
    return n, per, nk - (n - 1) * per, rows - (nk - 1) * 32


def group_splits(problems, rows):                      # gemm_lin.hip group_splits (target = 0)
    tiles, nk = tiles128(problems), cdiv(rows, 32)
    smax = max(1, nk // 16)
    best, s = -1.0, 1
    for c in range(1, smax + 1):
        wgs = tiles * c
        eff = wgs / (512.0 * cdiv(wgs, 512))
        if eff > best + 0.02:
            best, s = eff, c
    return split_class(s, rows)


def group_slab_floats(problems, rows):                 # gemm_lin.hip gemm_tn_group_slab_floats
    return group_splits(problems, rows)[0] * sum(m * n + m for m, n in problems)


def tn_splits(m, n, rows):                             # gemm_lin.hip tn_splits
    nk = cdiv(rows, 32)
    s = max(1, min(512 // tiles128([(m, n)]), nk // 8))
    return split_class(s, rows)


def tn_slab_floats(m, n, rows):                        # gemm_lin.hip gemm_tn_slab_floats
    s = tn_splits(m, n, rows)[0]
    return (s * m * n if s > 1 else 0) + s * m


def bulk_tile(rows, n):                                # gemm_lin.hip lin_gemm (no deferred splits in these launches)
    return rows * n >= 128 * 128 * 256


def light(row):                                        # rau_ctx.h chain_bound()
    return row.mode == "eval" or row.dtype == "bf16" or row.B <= 64


def side_split(row):                                   # rau_ctx.h side_split(), rau_create reads the variable
    return row.env["RAU_SIDE_SPLIT"] != "0" if "RAU_SIDE_SPLIT" in row.env else light(row)


def enc_ws(row, d):                                    # enc_ws.hip enc_ws_ok (ER = 512), rau_ctx.hip plan_batch
    return d["Rq"] == 512 and row.B % 16 == 0 and row.B <= (64 if row.mode == "eval" else 32)


def enc_chunks(row, d, TL):                            # rau_ctx.hip encoder_forward, kEncHeadTokens = kEncSideChunks = 4
    if enc_ws(row, d) or not side_split(row) or TL <= 4:
        return ()
    nchunk = max(1, min(4, TL - 4))
    per = cdiv(TL - 4, nchunk)
    return tuple(min(per, TL - t0) for t0 in range(4, TL, per))


def hop_groups(row):                                   # rau_ctx.hip plan_batch; rau_forward: evaluate mode is one group
    H = row.H
    if row.mode == "eval" or row.B <= 64:
        return (H,)
    if H == 2:
        return (1, 1)
    sizes, left = [], H
    while left > 3:
        sizes.append(2)
        left -= 2
    return tuple(sizes + [1] * left)


def backward_schedule(row):                            # rau_ctx.hip backward_impl / group_conv_grads
    """(hops per conv-gradient group in launch order, (hops per side-stream q_proj_dgrad, hops left to the chain))"""
    HA, starts, h0 = active(row), {}, 0
    for g in hop_groups(row):
        starts[h0] = g
        h0 += g
    conv, side, left = [], [], HA
    for h in range(HA - 1, -1, -1):
        if h not in starts:
            continue
        n = min(h + starts[h], HA) - h
        if h > 0 and side_split(row):
            side.append(n)
            left = h
        conv.append(n)
    if row.mode == "eval":                             # I shared: one group, a conv launch per active hop
        conv = [1] * HA
    return tuple(conv), (tuple(side), left)


def ws_side_floats(row, d):                            # rau_ctx.hip plan_batch: p->ws[2]
    B, Q = row.B, 4 * d["Rq"]
    Sp = (d["S"] + 3) & ~3
    rowsH, rowsT = row.H * B, row.T * B
    sl = 16 * B * max(4 * d["R"], 4 * d["Rq"], d["K"], Q, d["M"], d["A"], Sp)
    shapes = [(d["K"], d["M"], rowsH), (d["M"], d["R"], rowsH), (4 * d["R"], d["M"], rowsH), (4 * d["R"], d["R"], rowsH),
              (d["M"], Sp, rowsH), (Sp, d["R"], rowsH), (d["A"], d["M"], rowsH), (d["M"], Q, rowsH),
              (4 * d["Rq"], d["E"], rowsT), (4 * d["Rq"], d["Rq"], rowsT)]
    sl = max([sl] + [tn_slab_floats(*s) for s in shapes])
    grp = max([group_slab_floats(mult_problems(d), hh * B) for hh in range(1, row.H + 1)] +
              [group_slab_floats(enc_problems(d), tt * B) for tt in range(1, row.T + 1)])
    return max(sl, grp)


def head_launches(row, d):                             # rau_ctx.hip rau_forward / forward_heads
    head_max = max(1, ws_side_floats(row, d) // 4 // (row.B * d["K"]))
    out = []
    for g in hop_groups(row):
        out += [min(head_max, g - h0) for h0 in range(0, g, head_max)]
    return head_max, tuple(out)


def colsum(rows):                                      # kernels.hip colsum_acc, kColChunks = 32 (N, ld % 4 == 0 here)
    per = cdiv(rows, 32)
    return ("v4" if rows >= 128 else "scalar"), sum(1 for c in range(32) if c * per >= rows and rows >= 128)


def classes(row):
    """Everything the rules above say about a row's step, in the table's words."""
    d = dims_of(row)
    B, HA, TL = row.B, active(row), row.TL
    mp, ep = mult_problems(d), enc_problems(d)
    conv_n, qd = backward_schedule(row)
    head_max, heads = head_launches(row, d)
    chunks = enc_chunks(row, d, TL)
    t_head = 4 if chunks else TL
    return dict(
        mult=group_splits(mp, HA * B) if HA else None,
        enc=group_splits(ep, TL * B) if TL else None,
        mult_max=max(group_splits(mp, hh * B)[0] for hh in range(1, row.H + 1)),
        enc_max=max(group_splits(ep, tt * B)[0] for tt in range(1, row.T + 1)),
        chunks=chunks, i2h=(1 + len(chunks)) if TL else 0,
        groups=hop_groups(row), conv_n=conv_n, qd=qd,
        head_max=head_max, heads=heads,
        rows=HA * B, colsum=colsum(HA * B),
        q_bulk=bulk_tile(qd[1] * B, 4 * d["Rq"]), i2h_bulk=bulk_tile(t_head * B, 4 * d["Rq"]))


NEEDS = {"split": ({"mult"}, {"enc"}), "enc": ({"chunks"},), "empty": ({"chunks", "i2h"},),
         "hops": ({"groups", "conv_n", "qd"},), "heads": ({"head_max", "heads"},), "tiles": ({"rows", "colsum"},),
         "bulk": ({"q_bulk", "i2h_bulk"},), "bf16": ({"mult", "enc"}, {"chunks"}, {"groups", "conv_n", "qd"})}


@pytest.mark.parametrize("row", CASES, ids=[f"{r.sec}-{row_id(r)}" for r in CASES])
def test_a_row_states_what_the_rules_give(row):
    got = classes(row)
    assert row.cls and {k: got[k] for k in row.cls} == row.cls
    assert any(need <= set(row.cls) for need in NEEDS[row.sec]), "the row does not state its section's class"
    assert row.why and 0 <= row.TL <= row.T and (row.hop_w is None or len(row.hop_w) == row.H)
    d = dims_of(row)
    assert all(d[k] % 4 == 0 for k in ("E", "Rq", "D", "M", "A", "R", "K"))      # rau_create's rule
    assert not enc_ws(row, d)                          # tests/test_gpu_enc_ws.py holds the persistent encoder


def test_rows_are_distinct_and_of_a_known_section():
    ids = [(r.sec, row_id(r)) for r in CASES]
    assert len(set(ids)) == len(ids)
    assert {r.sec for r in CASES} == set(NEEDS)
    assert 60 <= len(CASES) + len(MODULE_B) <= 120


def some(pred, sec=None, **kw):
    return any(pred(r, classes(r)) for r in CASES
               if (sec is None or r.sec == sec) and all(getattr(r, k) == v for k, v in kw.items()))


def test_the_issue_s_split_counts():
    """The figures the rows of section 1 were chosen by, from the restatement alone."""
    base = dict(dims_of(CASES[0]))
    mp, ep = mult_problems(base), enc_problems(base)
    assert tiles128(mp) == 9 and tiles128(ep) == 4
    assert group_splits(mp, 8 * 261) == (3, 22, 22, 8) and group_splits(mp, 5 * 261) == (1, 41, 41, 25)
    assert group_splits(ep, 17 * 131) == (4, 18, 16, 19) and group_splits(ep, 15 * 131)[0] == 1
    wide = dict(base, Rq=512)
    mp, ep = mult_problems(wide), enc_problems(wide)
    assert group_splits(mp, 8 * 260) == (4, 17, 14, 32) and group_splits(mp, 5 * 260) == (2, 21, 20, 20)
    assert group_splits(ep, 13 * 260) == (2, 53, 53, 20) and group_splits(ep, 11 * 260) == (2, 45, 45, 12)
    # no split below 32 K-steps (993 rows), whatever the tile count
    assert all(group_splits(p, 992)[0] == 1 for p in (mp, ep, mult_problems(base), enc_problems(base)))
    assert group_splits(mp, 993)[0] == 2


def test_section_1_has_every_split_class_in_both_groups():
    for grp in ("mult", "enc"):
        own = lambda pred: some(lambda r, c: grp in r.cls and c[grp] is not None and pred(r, c[grp], c), sec="split")
        assert own(lambda r, g, c: g[0] == 1 and g[3] != 32), grp                      # unsplit, partial last step
        assert own(lambda r, g, c: g[0] >= 2 and g[3] != 32), grp                      # split, partial last step
        assert own(lambda r, g, c: g[0] >= 2 and g[2] < g[1]), grp                     # split, shorter last split
        assert own(lambda r, g, c: g[0] >= 2 and g[3] == 32), grp                      # split at rows % 32 == 0
        assert own(lambda r, g, c: g[0] < c[grp + "_max"] and grp + "_max" in r.cls), grp    # below the slab's maximum
    # still split, with fewer splits than the slab holds
    assert some(lambda r, c: 2 <= c["mult"][0] < c["mult_max"] and "mult_max" in r.cls, sec="split")
    # gated by the hop weights and by the question lengths
    assert some(lambda r, c: active(r) < r.H and c["mult"][0] < c["mult_max"], sec="split")
    assert some(lambda r, c: r.TL < r.T and c["enc"][0] < c["enc_max"], sec="split")
    # the bf16 variant of the group kernel: both groups split, a partial last step
    assert some(lambda r, c: c["mult"][0] >= 2 and c["enc"][0] >= 2 and c["mult"][3] != 32 and c["enc"][3] != 32, sec="bf16")
    # f32, train mode, above 64 samples
    assert all(r.dtype == "f32" and r.mode == "train" and r.B > 64 for r in CASES if r.sec == "split")


def test_section_2_has_every_chunk_schedule():
    want = {1: (), 4: (), 5: (1,), 8: (1, 1, 1, 1), 9: (2, 2, 1), 13: (3, 3, 3), 22: (5, 5, 5, 3), 26: (6, 6, 6, 4)}
    for mode in ("train", "eval"):
        for TL, chunks in want.items():
            assert some(lambda r, c: c["chunks"] == chunks and c["i2h"] == 1 + len(chunks), sec="enc", B=6, T=26,
                        TL=TL, mode=mode), (mode, TL)
        assert some(lambda r, c: c["i2h"] == 0 and c["enc"] is None, sec="empty", mode=mode, TL=0)
    # multi-token chunks, a short last chunk, fewer launches than chunks asked for
    assert some(lambda r, c: len(c["chunks"]) == 3 and c["chunks"][-1] < c["chunks"][0], sec="enc")
    assert some(lambda r, c: len(c["chunks"]) == 4 and c["chunks"][-1] < c["chunks"][0], sec="enc")
    # the same TL where the context is not light: no chunks
    for TL in (9, 26):
        assert some(lambda r, c: not light(r) and c["chunks"] == () and c["i2h"] == 1, sec="enc", TL=TL), TL
    assert some(lambda r, c: len(c["chunks"]) > 1 and max(c["chunks"]) > 1, sec="bf16")
    # the sequence: a long TL in front of a short one, both modes, an empty batch in the middle
    tls = [tl for tl, _ in SEQUENCE]
    assert tls == [26, 5, 13, 0, 9, 3, 22] and {m for _, m in SEQUENCE} == {"train", "eval"}
    assert all(a != b for (_, a), (_, b) in zip(SEQUENCE, SEQUENCE[1:]))


def test_section_3_has_every_partition_and_every_end_of_the_active_hops():
    want = {3: (1, 1, 1), 5: (2, 1, 1, 1), 6: (2, 2, 1, 1), 7: (2, 2, 1, 1, 1), 8: (2, 2, 2, 1, 1)}
    plain = dict(sec="hops", over={}, env={})
    for H, groups in want.items():
        starts = [sum(groups[:i]) for i in range(len(groups))]
        two = [s for s, g in zip(starts, groups) if g == 2]
        assert some(lambda r, c: c["groups"] == groups and active(r) == H and r.hop_w is None, H=H, **plain), H
        assert some(lambda r, c: active(r) == 1, H=H, **plain), H
        assert some(lambda r, c: active(r) == H and r.hop_w is not None and 0.0 in r.hop_w, H=H, **plain), H
        assert some(lambda r, c: active(r) in starts[1:], H=H, **plain), H             # ends with a whole group
        if two:                                                                        # ends inside a two-hop group
            assert some(lambda r, c: active(r) - 1 in two and 1 in c["conv_n"][:1], H=H, **plain), H
        if len(two) > 1:                                                               # ... that is not the first
            assert some(lambda r, c: active(r) - 1 in two[1:], H=H, **plain), H
    assert all(r.B == 66 and r.mode == "train" for r in CASES if r.sec == "hops")
    # n = B in a two-hop group on the 14 x 14 kernels, and its control
    assert some(lambda r, c: r.over.get("S") == 196 and active(r) == 1 and c["groups"][0] == 2, sec="hops", H=5)
    assert some(lambda r, c: r.over.get("S") == 196 and active(r) == 5, sec="hops", H=5)
    # the side split above 64 samples: per-group launches, one of them over half a group
    assert some(lambda r, c: r.env and c["qd"] == ((1, 1, 2, 2), 2), sec="hops", H=8)
    assert some(lambda r, c: r.env and c["qd"][0][0] == 1 and c["groups"][2] == 2 and active(r) == 5, sec="hops", H=8)
    assert some(lambda r, c: not r.env and c["qd"][0] and active(r) < r.H, sec="bf16")


def test_section_4_flushes_inside_a_group_in_both_modes():
    for mode in ("train", "eval"):
        for merge in (None, (1.0, 1.0)):
            for heads in ((4,), (4, 1), (4, 2), (4, 4)):
                assert some(lambda r, c: c["heads"] == heads and c["head_max"] == 4 and c["groups"] == (r.H,),
                            sec="heads", mode=mode, merge=merge), (mode, merge, heads)
    for H in (4, 5, 6, 8):                             # the rows the issue names, whatever their class
        for merge in (None, (1.0, 1.0)):
            assert some(lambda r, c: True, sec="heads", B=6, H=H, mode="train", merge=merge)
            assert some(lambda r, c: True, sec="heads", B=66, H=H, mode="eval", merge=merge)
    assert some(lambda r, c: c["head_max"] == 7 and c["heads"] == (7, 1), sec="heads", B=6)
    d = dims_of(next(r for r in CASES if r.sec == "heads"))
    assert d["K"] == max(4 * d["R"], 4 * d["Rq"], d["K"], d["M"], d["A"], d["S"])


def test_section_5_has_both_sides_of_every_row_edge():
    got = {c["rows"]: c["colsum"] for r in CASES if r.sec == "tiles" for c in [classes(r)]}
    assert {63, 64, 65, 127, 128, 129} <= set(got)
    assert got[127] == ("scalar", 0) and got[128] == ("v4", 0) and got[129][0] == "v4" and got[129][1] > 0
    for B in (63, 64, 65, 127, 128, 129):
        assert some(lambda r, c: True, sec="tiles", B=B, H=1), B
    assert some(lambda r, c: c["rows"] == 129, sec="tiles", B=43, H=3)
    assert some(lambda r, c: c["groups"] == (1,) and light(r), sec="tiles", B=64)
    assert some(lambda r, c: not light(r), sec="tiles", B=65)
    for q, i in ((True, True), (False, True), (True, False)):
        assert some(lambda r, c: (c["q_bulk"], c["i2h_bulk"]) == (q, i) and "q_bulk" in r.cls and not side_split(r)), (q, i)
    # the two launches at the rows next to the edge
    assert bulk_tile(8 * 260, 2048) and not bulk_tile(7 * 260, 2048)
    assert some(lambda r, c: True, sec="bulk", TL=7) and some(lambda r, c: True, sec="bulk", TL=8)
    assert some(lambda r, c: active(r) == 7, sec="bulk") and some(lambda r, c: active(r) == 8 and "q_bulk" in r.cls)


def test_section_7_splits_the_module_level_gradients():
    d = MODULE_DIMS
    for B, want in MODULE_B.items():
        for m, n in mult_problems(d) + enc_problems(d):                  # every Linear has one tile at these widths
            assert tn_splits(m, n, B) == want, (B, m, n)
    got = {v[0] for v in MODULE_B.values()}
    assert got == {1, 2}
    assert any(s == 2 and tail != 32 and last < per for s, per, last, tail in MODULE_B.values())
    assert MODULE_B[480][0] == 1 and tn_splits(32, 32, 481)[0] == 2      # the last row count without a split
