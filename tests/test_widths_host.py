"""tests/test_gpu_widths.py's CASES table held to the dispatch predicates, without a device.

The conv kernels have no profile class of their own, so the table's "which kernel" columns cannot be asserted
where they run.  Here each predicate is restated in a few lines (from the file named beside it), every row's
stated kernels are compared with what the restatement gives, and the coverage the table claims -- each predicate
on both sides, each named edge on both sides -- is asserted, so that a row taken out of the table fails here.
"""
import pytest

from tests.test_gpu_widths import CASES, H, LIN_CALLS, LIN_DEPTH, LIN_N_OK, MODULE_WIDTHS, S, dims_of, row_id


# ---------------------------------------------------------------- the predicates, restated
def conv_wide_ok(rows, red, s=S):                      # conv_wide.hip (weight pitch = rows)
    return s == 196 and rows % 64 == 0 and red % 8 == 0 and red >= 16 and rows % 4 == 0


def conv_sample_ok(s, which, mask=12):                 # gemm_sample.hip, RAU_CONV_SAMPLE's default
    return bool(mask & which) and s % 4 == 0 and 176 < s <= 208


def conv_dz_fused_ok(s, m, bf16):                      # gemm_conv.hip
    return bf16 != 2 and m % 4 == 0 and conv_sample_ok(s, 4)


def light(row):                                        # rau_ctx.h chain_bound(); also LinMode::deep
    return row.mode == "eval" or row.dtype == "bf16" or row.B <= 64


def dgrad_dma_ok(m, a, s=S):                           # dgrad_dma.hip (weight pitch = m)
    return s == 196 and m % 128 == 0 and a % 16 == 0 and a >= 48 and m % 4 == 0


def wgrad_dma_ok(ra, rb, s=S):                         # wgrad_dma.hip
    return s == 196 and ra % 128 == 0 and rb % 128 == 0


def dgrad16_ok(m, a, s=S):                             # dgrad16.hip
    return s == 196 and m % 128 == 0 and a % 32 == 0 and a >= 32 and m % 4 == 0


def wgrad16_ok(ra, rb, s=S):                           # wgrad16.hip
    return s == 196 and ra >= 128 and rb >= 256 and ra % 128 == 0 and rb % 256 == 0


def att_dma_ok(m, a, s=S):                             # kernels.hip att_fwd_dma_ok / att_bwd_dma_sizes; at S = 196
    return s % 4 == 0 and s <= 256 and a <= 512 and m <= 512   # the LDS requests (58 - 68 KB) are below 96 KB


def family_split(row):                                 # rau_ctx.hip att_family_split
    return "RAU_ATT_SPLIT" in row.env or (row.B <= 64 and "RAU_ATT_FUSED" not in row.env)


def ds16_allocated(row):                               # rau_ctx.hip: bf16 mode, unpitched map
    return row.dtype == "bf16" and conv_dz_fused_ok(S, row.M, 1) and dgrad16_ok(row.M, row.A) and att_dma_ok(row.M, row.A)


def samples_per_launch(row):                           # rau_ctx.hip plan_batch / rau_forward
    if row.mode == "eval":
        return row.B                                   # I shared by the hops
    return H * row.B if row.B <= 64 else row.B         # one group of H hops; H = 2 above: a group per hop


def stage_depth(deep, k):                              # skinny_dma.hip
    return 32 if deep and k % 64 == 0 else 16


def ragged(deep, k, brc, n):
    return k % (2 * stage_depth(deep, k)) != 0 or (brc and n % 64 != 0)


# ---------------------------------------------------------------- what a row's step launches
def dispatch(row):
    D, M, A = row.D, row.M, row.A
    bf16, train = row.dtype == "bf16", row.mode == "train"
    n = samples_per_launch(row)
    dzf = conv_dz_fused_ok(S, M, int(bf16))
    x16 = bf16 and train and dzf                       # xd16, and the mask that makes the hop copies
    ds16 = ds16_allocated(row) and train and not family_split(row) and dzf

    def fwd(rows, red):
        if bf16:
            return "b16" if x16 else "bf16"
        if conv_wide_ok(rows, red) and n >= 4:
            return "wide" if n % 4 == 0 else "wide+tail"
        assert not conv_sample_ok(S, 1) and not conv_sample_ok(S, 2)
        return "general"
    if not train:
        dgrad = "sample" if M % 4 == 0 and conv_sample_ok(S, 4) else "general"
    elif bf16:
        dgrad = ("dgrad16+dS16" if ds16 else "dgrad16") if dgrad16_ok(M, A) else "sample+dZ16"
    else:
        dgrad = "dgrad_dma" if not light(row) and dgrad_dma_ok(M, A) else "sample+dZ"
    if bf16:
        wg_att = "ds16" if ds16 else "32bf16"
        wg_emb = ("wgrad16" if wgrad16_ok(M, D) else "b16") if x16 else "32bf16dtanh"
    else:
        wg_att = "dma" if wgrad_dma_ok(A, M) else "28"
        wg_emb = ("dma" if wgrad_dma_ok(M, D) else "28") if train and dzf else "28dtanh"
    att = "split" if family_split(row) else "fused" if att_dma_ok(M, A) else "fused_regs"
    return f"{fwd(M, D)} {fwd(A, M)}", dgrad, f"{wg_att} {wg_emb}", att


@pytest.mark.parametrize("row", CASES, ids=[f"{r.sec}-{row_id(r)}" for r in CASES])
def test_a_row_states_what_the_predicates_give(row):
    assert (row.fwd, row.dgrad, row.wgrad, row.att) == dispatch(row)
    assert row.why and all(v % 4 == 0 for v in (row.D, row.M, row.A))     # rau_create's rule


def test_rows_are_distinct_and_of_a_known_section():
    ids = [(r.sec, row_id(r)) for r in CASES]
    assert len(set(ids)) == len(ids)
    assert {r.sec for r in CASES} == {"small", "large", "fused6", "batch", "bf16", "lin"}
    assert 60 <= len(CASES) + len(MODULE_WIDTHS) <= 130


def some(pred, sec=None, **kw):
    return any(pred(r) for r in CASES if (sec is None or r.sec == sec) and all(getattr(r, k) == v for k, v in kw.items()))


F32T = dict(dtype="f32", mode="train")


def test_every_predicate_is_true_and_false_somewhere():
    for want in (True, False):
        assert some(lambda r: conv_wide_ok(r.M, r.D) == want, dtype="f32"), want          # i_embed
        assert some(lambda r: conv_wide_ok(r.A, r.M) == want, dtype="f32"), want          # ifeatproj
        assert some(lambda r: (samples_per_launch(r) >= 4) == want, dtype="f32"), want
        assert some(lambda r: light(r) == want, **F32T), want
        assert some(lambda r: not light(r) and dgrad_dma_ok(r.M, r.A) == want, **F32T), want
        assert some(lambda r: wgrad_dma_ok(r.A, r.M) == want, dtype="f32"), want
        assert some(lambda r: wgrad_dma_ok(r.M, r.D) == want, **F32T), want
        assert some(lambda r: dgrad16_ok(r.M, r.A) == want, dtype="bf16", mode="train"), want
        assert some(lambda r: wgrad16_ok(r.M, r.D) == want, dtype="bf16", mode="train"), want
        assert some(lambda r: not family_split(r) and att_dma_ok(r.M, r.A) == want, dtype="f32"), want
        assert some(lambda r: not family_split(r) and att_dma_ok(r.M, r.A) == want, dtype="bf16"), want
        assert some(lambda r: ds16_allocated(r) == want, dtype="bf16", mode="train"), want
        assert some(lambda r: family_split(r) == want, dtype="f32"), want
        assert some(lambda r: family_split(r) == want, dtype="bf16"), want
    # by its mask the per-sample tile takes the attention dgrad and not the forward convs
    assert conv_sample_ok(S, 4) and conv_sample_ok(S, 8) and not conv_sample_ok(S, 1) and not conv_sample_ok(S, 2)
    # conv_dz_fused_ok has no false side at S = 196 in these two dtypes: rau_create asks for M % 4
    assert all(conv_dz_fused_ok(S, r.M, int(r.dtype == "bf16")) for r in CASES)
    # each weight gradient takes wgrad_dma while the other does not
    assert some(lambda r: wgrad_dma_ok(r.A, r.M) and not wgrad_dma_ok(r.M, r.D), **F32T)
    assert some(lambda r: not wgrad_dma_ok(r.A, r.M) and wgrad_dma_ok(r.M, r.D), **F32T)
    # dgrad16 and wgrad16 each alone, both, neither
    for d16 in (True, False):
        for w16 in (True, False):
            assert some(lambda r: (dgrad16_ok(r.M, r.A), wgrad16_ok(r.M, r.D)) == (d16, w16), sec="bf16", mode="train")
    assert some(lambda r: True, sec="bf16", mode="eval")
    # 16-bit dS in use (fused family) and allocated but unused (split family)
    assert some(lambda r: r.dgrad == "dgrad16+dS16", sec="bf16") and some(lambda r: ds16_allocated(r) and family_split(r))


def test_the_named_edges_have_a_row_on_both_sides():
    ctl = dict(M=128, A=128)
    # conv_wide: two K-steps and the width below; an odd count; % 4 but not % 8 with rows % 64; three row tiles
    for D in (16, 8, 24, 132):
        assert some(lambda r: True, sec="small", D=D, **ctl, **F32T), D
    assert some(lambda r: r.M % 8 == 4 and r.A % 64 == 0 and r.D % 8 == 0, sec="small", **F32T)
    assert some(lambda r: r.M == 192 and r.A == 192, sec="small", **F32T)
    for r_ in (96,):                                   # rows % 64 != 0, reduction eligible
        assert some(lambda r: r.M == r_ and r.D % 8 == 0, sec="small", **F32T)
        assert some(lambda r: r.A == r_ and r.M % 8 == 0, sec="small", **F32T)
    # dgrad_dma, not light: the ring's minimum and below, odd stages, A % 16, row tiles, M % 128
    for A in (48, 32, 80, 72):
        assert some(lambda r: not light(r), sec="large", D=128, M=128, A=A), A
        assert some(lambda r: light(r), sec="small", D=128, M=128, A=A, **F32T), A    # the per-sample tile there
    for M in (384, 192):
        assert some(lambda r: not light(r), sec="large", D=128, M=M, A=128), M
    assert some(lambda r: not light(r) and dgrad_dma_ok(r.M, r.A) and (r.A // 16) % 2 == 1 and r.A > 48)
    # wgrad_dma: non-square grids at a large batch, and a grid whose split count is not the sample count
    grid = lambda ra, rb: (ra // 128, rb // 128)
    assert some(lambda r: grid(r.A, r.M) == (1, 3) and grid(r.M, r.D) == (3, 1), sec="large")
    assert some(lambda r: grid(r.M, r.D) == (1, 2), sec="large")
    tiles = lambda r: (r.A // 128) * (r.M // 128)
    for two_groups in (True, False):                   # wgrad_dma.hip: two wave groups up to 8 tiles
        assert some(lambda r: wgrad_dma_ok(r.A, r.M) and 512 // tiles(r) < r.B and (tiles(r) <= 8) == two_groups, sec="large")
    # the attention width edge, in both batch classes, with the class asserted on the device
    for sec in ("large", "fused6"):
        for M, A in ((128, 512), (128, 516), (128, 640), (516, 128), (640, 128)):
            assert some(lambda r: not family_split(r), sec=sec, M=M, A=A), (sec, M, A)
    assert some(lambda r: family_split(r) and r.A > 512, sec="small") and some(lambda r: family_split(r) and r.M > 512, sec="small")
    # dgrad16 / wgrad16
    b16 = dict(sec="bf16", mode="train")
    for A in (32, 48):
        assert some(lambda r: True, D=256, M=256, A=A, **b16), A
    for M in (128, 384, 192):
        assert some(lambda r: True, D=256, M=M, A=64, **b16), M
    for D in (512, 384):
        assert some(lambda r: True, D=D, M=256, A=64, **b16), D
    # samples per launch: none wide, no tail, and each remainder, in train mode and in evaluate mode
    for mode in ("train", "eval"):
        n_of = lambda pred: some(lambda r: pred(samples_per_launch(r)), sec="batch", mode=mode)
        assert n_of(lambda n: n < 4) and n_of(lambda n: n >= 4 and n % 4 == 0), mode
        for rem in (1, 2, 3) if mode == "train" else (1, 3):
            assert n_of(lambda n: n > 4 and n % 4 == rem), (mode, rem)
    assert some(lambda r: samples_per_launch(r) == 4, sec="batch")
    for B in (3, 4, 5, 7, 64, 65):
        assert some(lambda r: True, sec="batch", B=B, D=128, **ctl, **F32T), B
    assert some(lambda r: True, sec="batch", B=64, att="split", dgrad="sample+dZ")
    assert some(lambda r: True, sec="batch", B=65, att="fused", dgrad="dgrad_dma")
    chunks = lambda r: 8 if r.B <= 64 else 4           # kernels.hip att_chunks, split family only
    assert {chunks(r) for r in CASES if r.sec == "batch" and family_split(r) and r.B >= 64} == {4, 8}
    assert some(lambda r: r.M == 512 and not family_split(r) and att_dma_ok(r.M, r.A))
    # the module-level widths are rows of the table
    for D, M, A in MODULE_WIDTHS:
        assert some(lambda r: True, sec="small", D=D, M=M, A=A, **F32T), (D, M, A)


def lin_classes(row):
    """{(form, class)} over the Linear products of a row; class: '32', '16' (not ragged), 'rag'."""
    d = dict(dims_of(row), S=S)
    deep = light(row)
    out = set()
    for _, form, n_expr, k_expr in LIN_CALLS:
        n, k = eval(n_expr, {}, d), eval(k_expr, {}, d)
        brc = form == "nn"
        cls = "rag" if ragged(deep, k, brc, n) else str(stage_depth(deep, k))
        # the table's statement, for deep launches: by reduction length, and by N for [K][N] weights
        if deep:
            assert LIN_DEPTH[k] == ("rag" if ragged(deep, k, False, 64) else str(stage_depth(deep, k))), (k, row)
            assert LIN_N_OK[n] == (n % 64 == 0), (n, row)
            assert cls == (LIN_DEPTH[k] if not brc or LIN_N_OK[n] else "rag")
        out.add((form, cls))
    return out


def test_linear_rows_reach_every_class_in_both_forms_and_both_dtypes():
    for dtype in ("f32", "bf16"):
        got = set()
        for r in CASES:
            if r.sec == "lin" and r.dtype == dtype and light(r):
                got |= lin_classes(r)
        assert got == {(f, c) for f in ("nt", "nn") for c in ("32", "16", "rag")}, (dtype, got)
    # each width's own class, on the reduction over R
    for w, cls in ((64, "32"), (96, "16"), (100, "rag")):
        assert LIN_DEPTH[w] == cls
        for dtype in ("f32", "bf16"):
            assert some(lambda r: r.over == dict(R=w, Rq=w, K=w) and light(r), sec="lin", dtype=dtype), (w, dtype)
    # and a launch that is not deep: % 64 reductions on 16-deep stages
    shallow = [r for r in CASES if r.sec == "lin" and not light(r)]
    assert shallow and all(("nt", "16") in lin_classes(r) and ("nt", "32") not in lin_classes(r) for r in shallow)
