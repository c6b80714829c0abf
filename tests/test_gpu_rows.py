"""Parity over the row counts of the recurrence's side: B, HA B and TL B (HA = active hops, TL = longest question).

tests/test_gpu_positions.py sweeps the position count and tests/test_gpu_widths.py the channel widths; the third axis
of the dispatch is the number of ROWS the Linear GEMMs, the grouped weight gradients, the column sums, the encoder's
token schedule, the hop-group schedule and the head launches get.  All of it is reachable at tiny widths (BASE below),
where the fp64 autograd oracle of B = 261, H = 8 takes about a second.  The predicates, read off the code at this
commit (tests/test_rows_host.py restates them and holds CASES below to them):

  predicate (file)                      condition on the rows
  group_splits (gemm_lin.hip)           the grouped Linear weight gradients: nine mult-group problems over HA B rows,
      four encoder problems over TL B rows, one launch each.  nk = ceil(rows / 32) K-steps; at most nk / 16 splits, so
      none below 993 rows; the count is the one that fills whole rounds of 512 workgroups best (+0.02 hysteresis);
      per = ceil(nk / s) steps per split: the last split may be shorter, the last step partial (rows % 32).
      plan_batch (rau_ctx.hip) sizes the slab as the maximum over hh = 1..H and tt = 1..T: a gated step or a short TL
      takes another split count inside that slab.
  tn_splits (gemm_lin.hip)              the module-level weight gradients over B rows: min(512 / tiles, nk / 8) splits.
  lin_gemm (gemm_lin.hip)               one unsplit 128 x 128 launch where rows x N >= 128 * 128 * 256: q_proj_dgrad
      (rows the chain still owes x 4 Rq) and enc_i2h_gemm (TL B x 4 Rq) cross it at Rq = 512, B = 260.
  encoder_forward (rau_ctx.hip)         with the side split (chain_bound: evaluate mode, bf16 mode or up to 64 samples;
      RAU_SIDE_SPLIT overrides) and no persistent encoder, the layer-1 input projection of the tokens behind the first
      kEncHeadTokens = 4 runs on the third stream in min(4, TL - 4) chunks of ceil((TL - 4) / nchunk) tokens, each with
      its event; the recurrence waits for the chunk that starts with the token it is about to read.
  TL = 0                                no encoder launch at all, gather_q on zero states; the backward leaves the EMBED
      and RNN gradients alone.
  plan_batch groups (rau_ctx.hip)       above 64 samples in train mode: pairs while more than three hops are left, then
      single hops (H = 2: 1, 1).  A group's conv gradients get (min(h + g, HA) - h) B maps, its q_proj_dgrad (side split)
      as many rows on the third stream; the chain keeps the rows of the hops in front of the first such group.
  head_max (rau_ctx.hip rau_forward)    ws_side.floats / 4 / (B K) hops per head launch: a one-group context (up to
      64 samples, or evaluate mode) with more hops flushes the heads in the middle of the group and, in train mode,
      forms dpre / dhn of the flushed hops only.
  colsum_acc (kernels.hip)              float4 path from 128 rows on; 32 chunks of ceil(rows / 32) rows: chunks that
      start behind the last row exist from 129 rows on.

Where the plan these rows were chosen by (LOG.md) and the code differ, by the restatement (the rows the plan names
are all kept; rows were added so that the class it meant is reached as well):
  * head_max at B = 6, K = 256, M = 64 is 7, not 4: the side stream's workspace is sized by the grouped weight
    gradients' slab there (43.9 k floats against 16 B K = 24.6 k).  H = 8 flushes as 7 + 1.  B = 22 has head_max = 4
    (4 / 4 + 1 / 4 + 2 / 4 + 4) in train mode, B = 66 in evaluate mode.
  * tn_splits at B = 511: nk = ceil(511 / 32) = 16, so s = 2 (8 + 8 steps, a 31-row tail), not 1.  B = 480 is the
    last s = 1.

Bars, unchanged: f32 step path against the fp64 oracle tests/test_gpu_parity.check (1e-4 max-norm per output and per
layer slice of every gradient, argmax exact on decided rows); bf16 mode tests/test_gpu_bf16.run with its derived
bars; module level against the step path 2e-5 (tests/test_gpu_positions.module_level_feval).
"""
from collections import namedtuple

import numpy as np
import pytest

from tests import util
from tests import test_gpu_bf16, test_gpu_parity, test_gpu_positions

pytestmark = pytest.mark.gpu

BASE = dict(V=40, E=16, Rq=32, D=16, S=16, M=32, A=16, R=32, K=48)
SCALE = test_gpu_positions.SCALE
ENV = test_gpu_positions.ATT_ENV + ("RAU_SIDE_SPLIT", "RAU_HOP_GROUPS", "RAU_BWD_GROUPS", "RAU_ENC_CHUNKS", "RAU_WG_BULK")

# sec: the section that runs the row.  TL: the longest question of the batch (lens are drawn up to it, lens[0] = TL).
# hop_w: None = every hop weighted H.  cls: what the row is there for, in the words of tests/test_rows_host.classes():
#   mult, enc   (splits, K-steps per split, K-steps of the last split, rows of the last K-step; 32 = a full one) of the
#               two grouped weight-gradient launches; mult_max, enc_max: the largest split count the slab was sized for
#   chunks      tokens per third-stream launch of the layer-1 input projection, () = one launch on the chain
#   groups      the hop-group partition; conv_n: hops whose maps each group's conv gradients get, in launch order;
#               qd: (hops per q_proj_dgrad on the third stream in launch order, hops the chain's own launch has)
#   head_max, heads   hops per head launch, in launch order
#   rows, colsum      HA B and the stage-1 kernel of colsum_acc with its count of chunks behind the last row
#   q_bulk, i2h_bulk  the launch is one unsplit 128 x 128 tile grid
#   tn          (splits, steps per split, steps of the last, rows of the last step) of the module-level gradients
Row = namedtuple("Row", "sec B T H TL mode dtype hop_w cls why over env merge", defaults=({}, {}, None))
RQ512 = dict(Rq=512)
TILES11 = dict(K=304, Rq=96)                     # three 128-row tiles in cls, q_proj and every encoder Linear
SIDE = {"RAU_SIDE_SPLIT": "1"}
WIDE_K = dict(K=256, M=64)                       # K the widest of {4R, 4Rq, K, Q, M, A, S}
S196 = dict(S=196, D=128, M=128, A=128)          # tests/test_gpu_positions.py's shape: dgrad_dma / wgrad_dma


def w(H, *zeros, HA=None):
    """hop weights H with zeros behind HA and at the named hops"""
    return tuple(0.0 if (HA is not None and h >= HA) or h in zeros else float(H) for h in range(H))


CASES = [
    # ---- 1. grouped Linear weight gradients: K split over rows (f32, train mode, above 64 samples)
    Row("split", 261, 5, 8, 5, "train", "f32", None, dict(mult=(3, 22, 22, 8), enc=(1, 41, 41, 25)),
        "mult group split in three even parts with an 8-row last K-step; encoder group unsplit at rows % 32 != 0"),
    Row("split", 261, 5, 8, 5, "train", "f32", w(8, HA=5), dict(mult=(1, 41, 41, 25), mult_max=3),
        "hops 5..7 gated off: 1305 rows unsplit inside a slab sized for three splits"),
    Row("split", 131, 17, 8, 17, "train", "f32", None, dict(enc=(4, 18, 16, 19), mult=(1, 33, 33, 24)),
        "encoder group: four splits, a shorter last split (16 of 18 steps) and a 19-row last step"),
    Row("split", 131, 17, 8, 15, "train", "f32", None, dict(enc=(1, 62, 62, 13), enc_max=4),
        "lens capped at 15: 1965 rows unsplit inside a slab sized for four splits"),
    Row("split", 260, 13, 8, 13, "train", "f32", None, dict(mult=(4, 17, 14, 32), enc=(2, 53, 53, 20), q_bulk=True, i2h_bulk=True),
        "Rq = 512 (16 + 3 * 64 encoder tiles, 24 mult tiles): mult group 17 / 17 / 17 / 14 steps at rows % 32 == 0; "
        "encoder group two even splits with a 20-row tail; both bulk-tile launches above the edge", RQ512),
    Row("split", 260, 13, 8, 13, "train", "f32", w(8, HA=5), dict(mult=(2, 21, 20, 20), mult_max=4),
        "HA = 5: two splits of 21 / 20 steps with a 20-row tail, below the context's four", RQ512),
    Row("split", 260, 13, 8, 11, "train", "f32", None, dict(enc=(2, 45, 45, 12)),
        "TL = 11: encoder group two even splits with a 12-row tail", RQ512),
    Row("split", 256, 8, 8, 8, "train", "f32", None, dict(mult=(3, 22, 20, 32), enc=(4, 16, 16, 32)),
        "rows % 32 == 0 in both groups: 2048 rows, mult 22 / 22 / 20, encoder four even splits"),
    Row("split", 256, 8, 8, 8, "train", "f32", w(8, HA=7), dict(mult=(3, 19, 18, 32), mult_max=3),
        "HA = 7: 1792 rows, 19 / 19 / 18 steps"),
    Row("split", 261, 9, 8, 9, "train", "f32", None, dict(enc=(4, 19, 17, 13), mult=(3, 22, 22, 8)),
        "both groups split with a partial last step; encoder 19 / 19 / 19 / 17 with a 13-row tail"),
    Row("split", 261, 9, 8, 8, "train", "f32", w(8, 2), dict(enc=(4, 17, 15, 8), enc_max=4),
        "TL = 8 in the T = 9 context, an interior hop gated off: 17 / 17 / 17 / 15 steps"),
    Row("split", 261, 9, 8, 7, "train", "f32", None, dict(enc=(1, 58, 58, 3), enc_max=4),
        "TL = 7: 1827 rows unsplit, a 3-row last step"),
    Row("split", 125, 8, 8, 8, "train", "f32", None, dict(mult=(2, 16, 16, 8), enc=(2, 16, 16, 8)),
        "13 mult and 12 encoder tiles: from 11 tiles on two splits fill the rounds better, so both groups split at the "
        "first row count that allows it (32 K-steps), with an 8-row last step", TILES11),
    # ---- 2. the encoder's token schedule in light contexts (B = 6, T = 26)
    *[Row("enc", 6, 26, 2, TL, mode, "f32", None, dict(chunks=chunks), why)
      for TL, chunks, why in [(1, (), "one token: head launch only"), (4, (), "the head tokens exactly"),
                              (5, (1,), "one chunk of one token"), (8, (1, 1, 1, 1), "four one-token chunks"),
                              (9, (2, 2, 1), "per = 2: three launches for four chunks, a short last chunk"),
                              (13, (3, 3, 3), "per = 3, three launches"), (22, (5, 5, 5, 3), "per = 5, a short last chunk"),
                              (26, (6, 6, 6, 4), "per = 6 at the context's T")]
      for mode in ("train", "eval")],
    Row("enc", 66, 26, 2, 9, "train", "f32", None, dict(chunks=()), "not light: one enc_i2h_gemm, no chunks"),
    Row("enc", 66, 26, 2, 26, "train", "f32", None, dict(chunks=()), "not light at the context's T"),
    Row("empty", 5, 26, 2, 0, "train", "f32", None, dict(chunks=(), i2h=0), "every question empty: no encoder launch"),
    Row("empty", 5, 26, 2, 0, "eval", "f32", None, dict(chunks=(), i2h=0), "every question empty, evaluate mode"),
    # ---- 3. hop groups and gating above 64 samples (B = 66, f32, train mode)
    *[Row("hops", 66, 4, H, 4, "train", "f32", hw, dict(groups=groups, conv_n=conv_n, qd=qd), why)
      for H, groups, rows in [
          (3, (1, 1, 1), [(None, (1, 1, 1), ((), 3), "all hops"),
                          (w(3, HA=2), (1, 1), ((), 2), "HA = 2: the last group never starts"),
                          (w(3, HA=1), (1,), ((), 1), "HA = 1"),
                          (w(3, 1), (1, 1, 1), ((), 3), "an interior zero weight")]),
          (5, (2, 1, 1, 1), [(None, (1, 1, 1, 2), ((), 5), "all hops"),
                             (w(5, HA=4), (1, 1, 2), ((), 4), "HA = 4: ends with a one-hop group"),
                             (w(5, HA=2), (2,), ((), 2), "HA = 2: the two-hop group alone, whole"),
                             (w(5, HA=1), (1,), ((), 1), "HA = 1: inside the two-hop group, n = B"),
                             (w(5, 2), (1, 1, 1, 2), ((), 5), "an interior zero weight")]),
          (6, (2, 2, 1, 1), [(None, (1, 1, 2, 2), ((), 6), "all hops"),
                             (w(6, HA=3), (1, 2), ((), 3), "HA = 3: ends inside the second two-hop group, n = B"),
                             (w(6, HA=4), (2, 2), ((), 4), "HA = 4: at the first one-hop group's start"),
                             (w(6, HA=5), (1, 2, 2), ((), 5), "HA = 5: the first one-hop group is the last active"),
                             (w(6, HA=1), (1,), ((), 1), "HA = 1"),
                             (w(6, 3), (1, 1, 2, 2), ((), 6), "an interior zero weight")]),
          (7, (2, 2, 1, 1, 1), [(None, (1, 1, 1, 2, 2), ((), 7), "all hops"),
                                (w(7, HA=3), (1, 2), ((), 3), "HA = 3: inside the second two-hop group"),
                                (w(7, HA=4), (2, 2), ((), 4), "HA = 4: at a group's start"),
                                (w(7, HA=1), (1,), ((), 1), "HA = 1"),
                                (w(7, 0), (1, 1, 1, 2, 2), ((), 7), "hop 0 gated off")]),
          (8, (2, 2, 2, 1, 1), [(None, (1, 1, 2, 2, 2), ((), 8), "all hops"),
                                (w(8, HA=5), (1, 2, 2), ((), 5), "HA = 5: inside the third two-hop group"),
                                (w(8, HA=3), (1, 2), ((), 3), "HA = 3: inside the second"),
                                (w(8, HA=6), (2, 2, 2), ((), 6), "HA = 6: at the first one-hop group's start"),
                                (w(8, HA=7), (1, 2, 2, 2), ((), 7), "HA = 7"),
                                (w(8, HA=1), (1,), ((), 1), "HA = 1"),
                                (w(8, 4, 6), (1, 1, 2, 2, 2), ((), 8), "two interior zero weights")])]
      for hw, conv_n, qd, why in rows],
    Row("hops", 66, 4, 5, 4, "train", "f32", w(5, HA=1), dict(groups=(2, 1, 1, 1), conv_n=(1,), qd=((), 1)),
        "S = 196, D = M = A = 128: dgrad_dma / wgrad_dma with n = B in a two-hop group", S196),
    Row("hops", 66, 4, 5, 4, "train", "f32", None, dict(groups=(2, 1, 1, 1), conv_n=(1, 1, 1, 2), qd=((), 5)),
        "S = 196, D = M = A = 128: the control of the row above", S196),
    Row("hops", 66, 4, 8, 4, "train", "f32", None, dict(groups=(2, 2, 2, 1, 1), conv_n=(1, 1, 2, 2, 2), qd=((1, 1, 2, 2), 2)),
        "RAU_SIDE_SPLIT: every finished group's dq rows on the third stream, the chain keeps hops 0, 1", {}, SIDE),
    Row("hops", 66, 4, 8, 4, "train", "f32", w(8, HA=5), dict(groups=(2, 2, 2, 1, 1), conv_n=(1, 2, 2), qd=((1, 2), 2)),
        "RAU_SIDE_SPLIT with HA inside the third group: nh = 1 of a two-hop group", {}, SIDE),
    # ---- 4. heads per launch (K = 256 the widest width)
    *[Row("heads", B, 4, H, 4, mode, "f32", None, dict(head_max=hm, heads=heads), why, WIDE_K, {}, merge)
      for B, mode, hm, rows in [
          (6, "train", 7, [(4, (4,)), (5, (5,)), (6, (6,)), (8, (7, 1))]),
          (22, "train", 4, [(4, (4,)), (5, (4, 1)), (6, (4, 2)), (8, (4, 4))]),
          (66, "eval", 4, [(4, (4,)), (5, (4, 1)), (6, (4, 2)), (8, (4, 4))])]
      for H, heads in rows
      for merge, why in [(None, "heads " + " + ".join(map(str, heads))),
                         ((1.0, 1.0), "the same with merge_w: the backward forms dpre / dhn of all hops itself")]],
    # ---- 5. row tiles and the colsum switch (H = 1: HA B = B), the bulk-tile edge
    *[Row("tiles", B, 4, H, 4, "train", "f32", None, dict(rows=H * B, colsum=cs), why)
      for B, H, cs, why in [(63, 1, ("scalar", 0), "one 64-row tile, one row short"),
                            (64, 1, ("scalar", 0), "one full tile; last batch of the one-group context"),
                            (65, 1, ("scalar", 0), "a one-row second tile; first batch above the 64-sample switch"),
                            (127, 1, ("scalar", 0), "last row count of the scalar column sums"),
                            (128, 1, ("v4", 0), "first row count of the float4 column sums, 4 rows per chunk"),
                            (129, 1, ("v4", 6), "per = 5: six chunks start behind the last row; a one-row third tile"),
                            (43, 3, ("v4", 6), "129 rows as 3 x 43 in a one-group context")]],
    Row("bulk", 260, 13, 8, 13, "train", "f32", w(8, HA=7), dict(q_bulk=False, i2h_bulk=True),
        "q_proj_dgrad 1820 x 2048: below the edge", RQ512),
    Row("bulk", 260, 13, 8, 7, "train", "f32", None, dict(q_bulk=True, i2h_bulk=False),
        "enc_i2h_gemm 1820 x 2048: below the edge", RQ512),
    Row("bulk", 260, 13, 8, 8, "train", "f32", None, dict(q_bulk=True, i2h_bulk=True),
        "enc_i2h_gemm 2080 x 2048: the first TL above the edge", RQ512),
    # ---- 6. bf16 mode (light above 64 samples: the side split runs by default)
    Row("bf16", 125, 8, 8, 8, "train", "bf16", None, dict(mult=(2, 16, 16, 8), enc=(2, 16, 16, 8), chunks=(1, 1, 1, 1)),
        "section 1's smallest context with both groups split, on the bf16 group kernel: an 8-row last step in both "
        "(the reference's per-sample pass costs B backward passes: 1000 rows is what a split needs)", TILES11),
    Row("bf16", 6, 26, 2, 13, "train", "bf16", None, dict(chunks=(3, 3, 3)), "the chunked projection, bf16 products"),
    Row("bf16", 66, 4, 5, 4, "train", "bf16", w(5, HA=1), dict(groups=(2, 1, 1, 1), conv_n=(1,), qd=((), 1)),
        "HA inside the two-hop group"),
    Row("bf16", 66, 4, 8, 4, "train", "bf16", w(8, HA=5), dict(groups=(2, 2, 2, 1, 1), conv_n=(1, 2, 2), qd=((1, 2), 2)),
        "HA inside the third group with the default side split: q_proj_dgrad rows of a half group"),
]

# 7. module level: B -> tn_splits' (splits, steps per split, steps of the last split, rows of the last step)
MODULE_B = {523: (2, 9, 8, 11), 511: (2, 8, 8, 31), 480: (1, 15, 15, 32)}
MODULE_DIMS = dict(BASE, T=4, H=2)

# the one context that runs many TL in a row (section 2): (TL, mode)
SEQUENCE = [(26, "train"), (5, "eval"), (13, "train"), (0, "eval"), (9, "train"), (3, "eval"), (22, "train")]


def dims_of(row):
    return dict(BASE, B=row.B, T=row.T, H=row.H, **row.over)


def active(row):
    if row.merge is not None or row.hop_w is None:
        return row.H
    return max([h + 1 for h, v in enumerate(row.hop_w) if v != 0.0], default=0)


def row_id(row):
    extra = "".join(f"-{k}{v}" for k, v in sorted(row.over.items())) + "".join("-" + k[4:] for k in sorted(row.env))
    gated = "" if row.hop_w is None else "-w" + "".join("1" if v else "0" for v in row.hop_w)
    return (f"B{row.B}-T{row.T}-H{row.H}-TL{row.TL}-{row.mode}-{row.dtype}{gated}{extra}"
            + ("-merge" if row.merge else ""))


def rows(*secs, **kw):
    sel = [r for r in CASES if r.sec in secs and all(getattr(r, k) == v for k, v in kw.items())]
    return pytest.mark.parametrize("row", sel, ids=[row_id(r) for r in sel])


def lens_of(B, T, TL):
    """question lengths in [0, TL] with lens[0] = TL (the token buffers are T long)"""
    if TL == 0:
        return np.zeros(B, np.int32)
    lens = np.random.default_rng(100 * T + TL).integers(0, TL + 1, B).astype(np.int32)
    lens[0] = TL
    return lens


def hop_w_of(row):
    return np.array(row.hop_w if row.hop_w is not None else [float(row.H)] * row.H, np.float32)


def set_env(monkeypatch, row):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)               # read when the context is created


def profiled(monkeypatch, launched):
    """contexts made through model.RAU run with the profile on and leave their launch counts, by class, in `launched`"""
    from rau_vqa_amd import model

    class Profiled(model.RAU):
        def __init__(self, cfg):
            super().__init__(cfg)
            self.prof_enable()

        def close(self):
            self.sync()
            launched.update({k: v["launches"] for k, v in self.prof().items()})
            super().close()
    monkeypatch.setattr(model, "RAU", Profiled)


# ---------------------------------------------------------------- f32 step path against the fp64 oracle
_REFERENCES = {}


def check(monkeypatch, row, prof=False, torch_oracle=True):
    """tests/test_gpu_parity.check at the row; the fp64 reference of a problem is computed once for the rows that
    share it.  prof: as tests/test_gpu_positions.check, the launch counts by class are returned."""
    import oracle
    from oracle import ref_torch
    set_env(monkeypatch, row)
    dims, lens, hop_w = dims_of(row), lens_of(row.B, row.T, row.TL), hop_w_of(row)
    key = (row.mode, torch_oracle, tuple(sorted(dims.items())), row.TL, tuple(hop_w))
    mod = ref_torch if torch_oracle else oracle
    real_step = mod.step

    def step_once(*args, **kw):
        if key not in _REFERENCES:
            _REFERENCES[key] = real_step(*args, **kw)
        return _REFERENCES[key]
    monkeypatch.setattr(mod, "step", step_once)
    launched = {}
    if prof:
        profiled(monkeypatch, launched)
    errs = test_gpu_parity.check(util.shapes(dims), lens=lens, mode=row.mode, hop_w=hop_w, scale=SCALE,
                                 torch_oracle=torch_oracle)
    print(f"rows[{row.sec}] {row_id(row)}: largest error / bar {max(errs.values()) / test_gpu_parity.TOL:.4f}")
    return launched, _REFERENCES[key]


@rows("split")
def test_grouped_weight_gradients_split_over_rows(monkeypatch, row):
    """Section 1: one wgrad_gemm launch per group whatever the split; every layer's gradient against the oracle."""
    launched, _ = check(monkeypatch, row, prof=True)
    assert launched["wgrad_gemm"] == 2, launched


@rows("empty")
def test_every_question_empty(monkeypatch, row):
    """Section 2, TL = 0, against the C++ oracle (the autograd restatement has no encoder graph there): finite
    outputs, zero EMBED and RNN gradients (compared absolutely by check), a non-zero mult gradient."""
    launched, ref = check(monkeypatch, row, prof=True, torch_oracle=False)
    for cls in ("embed_fwd", "enc_i2h_gemm", "enc_h2h_gemm", "enc_h2h_dgrad", "enc_i2h_dgrad", "embed_bwd"):
        assert launched.get(cls, 0) == 0, launched
    assert launched["wgrad_gemm"] == 1 and launched["gather_q"] == 1, launched
    assert all(np.all(np.isfinite(ref[k])) for k in util.OUT_KEYS)
    assert not ref["g_embed"].any() and not ref["g_rnn"].any() and ref["g_mult"].any()


@rows("enc")
def test_encoder_token_schedule(monkeypatch, row):
    """Section 2: the chunked layer-1 input projection -- one launch on the chain and one per chunk, as the restated
    rule gives them."""
    launched, _ = check(monkeypatch, row, prof=True)
    assert launched["enc_i2h_gemm"] == 1 + len(row.cls["chunks"]), launched


def test_one_context_long_and_short_questions_in_a_row():
    """Section 2: T = 26, B = 6; TL = 26, 5, 13, 0, 9, 3, 22 on ONE context, train and evaluate mode alternating,
    every step against the oracle from scratch (tests/test_gpu_sequence.py's pattern): chunk events and
    enc_chunk_tok of a longer forward must not reach a shorter one.  The TL = 0 step accumulates on the step before
    it: its backward must leave the EMBED and RNN gradients as they were."""
    import oracle
    from oracle import ref_torch
    from rau_vqa_amd import synth
    from rau_vqa_amd.model import RAU, Config
    dims = dict(BASE, B=6, T=26, H=2)
    sh = util.shapes(dims)
    _, params, _ = util.make_problem(sh, scale=SCALE)
    m = RAU(Config(**{k: getattr(sh, k) for k in
                      ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H",
                       "p_we", "p_rnn", "p_q", "p_x", "p_mf")}))
    m.set_params(params)
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    acc, worst = None, 0.0
    for it, (TL, mode) in enumerate(SEQUENCE):
        batch = synth.make_batch(sh.B, sh.T, sh.V, sh.D, sh.S, sh.K, seed=500 + it, lens=lens_of(sh.B, sh.T, TL))
        masks = None
        if mode == "train":
            probs = {k: getattr(sh, "p_" + k) for k in oracle.MASK_SITES}
            masks = synth.make_masks(oracle.mask_shapes(sh), probs, seed=70 + it)
            m.training()
            m.set_masks(masks)
        else:
            m.evaluate()
        m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
        zero = TL != 0
        if zero:
            m.zero_grads()
        m.forward()
        out = m.outputs()
        m.backward(hop_w)
        g = m.get_grads()
        args = (sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks, hop_w)
        ref = ref_torch.step(*args) if TL else oracle.step(*args, dtype=np.float64)
        new = {k: np.asarray(ref["g_" + k], np.float64) for k in layouts}
        if not TL:
            assert not new["embed"].any() and not new["rnn"].any() and new["mult"].any()
        acc = new if zero else {k: acc[k] + new[k] for k in new}
        errs = {k: util.rel_err(out[k], ref[k]) for k in util.OUT_KEYS}
        for grp in layouts:
            for name, sl in util.layer_slices(layouts[grp]):
                r = acc[grp][sl]
                errs[name] = (float(np.max(np.abs(g[grp][sl] - r))) if np.max(np.abs(r)) < 1e-12
                              else util.rel_err(g[grp][sl], r))
        worst = max(worst, max(errs.values()))
        bad = {k: v for k, v in errs.items() if not v < test_gpu_parity.TOL}
        assert not bad, f"step {it} TL={TL} {mode}: {bad}"
    m.close()
    print(f"rows[enc] sequence: largest error / bar {worst / test_gpu_parity.TOL:.4f}")


def q_dgrad_launches(row):
    side, left = row.cls["qd"]
    return len(side) + (1 if left > 0 else 0)


@rows("hops")
def test_hop_groups_and_gating(monkeypatch, row):
    """Section 3: the partition of every H, HA ending inside a group, at a group's start, at one hop; the per-group
    q_proj_dgrad of the side split.  Launch counts from the profile: q_proj_dgrad, and the conv gradients' groups."""
    launched, _ = check(monkeypatch, row, prof=True)
    assert launched["q_proj_dgrad"] == q_dgrad_launches(row), launched
    assert launched["conv_att_dgrad"] == len(row.cls["conv_n"]), launched


def merged_check(monkeypatch, row, launched):
    """The row's step with merge_w through tests/merge_ref.py (tests/test_gpu_merged.py's parity, at the row)."""
    from tests import merge_ref
    from tests.test_gpu_merged import step
    from tests.test_gpu_select import GROUPS, grad_errs, make_model
    set_env(monkeypatch, row)
    profiled(monkeypatch, launched)
    sh = util.shapes(dims_of(row))
    batch, params, masks = util.make_problem(sh, lens=lens_of(row.B, row.T, row.TL), scale=SCALE)
    hop_w = hop_w_of(row)
    m = make_model(sh, params, masks if row.mode == "train" else None)
    if row.mode == "eval":
        m.evaluate()
        masks = None
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    got = step(m, hop_w, row.merge)
    dopred = m.dopred()
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = merge_ref.step(sh, params, batch, masks, hop_w, row.merge)
    assert np.array_equal(dopred > 0.5, ref["dopred"] > 0.5), "a do_pred crossed 0.5: the gates differ"
    errs = grad_errs(got, ref, layouts)
    print(f"rows[{row.sec}] {row_id(row)}: largest error / bar {max(errs.values()) / test_gpu_parity.TOL:.4f}")
    bad = {k: v for k, v in errs.items() if not v < test_gpu_parity.TOL}
    assert not bad, f"relative errors above {test_gpu_parity.TOL}: {bad}"


@rows("heads")
def test_heads_per_launch(monkeypatch, row):
    """Section 4: a one-group context with more hops than a head launch holds flushes in the middle of the group;
    two head_gemm per head launch.  In train mode the forward forms dpre / dhn of the flushed hops behind every flush
    (two head_dgrad each); in evaluate mode, and with merge_w in either mode, the backward forms them for all hops
    in one pair of launches."""
    launched = {}
    if row.merge is None:
        launched, _ = check(monkeypatch, row, prof=True)
    else:
        merged_check(monkeypatch, row, launched)
    heads = row.cls["heads"]
    assert sum(heads) == row.H and max(heads) <= row.cls["head_max"]
    assert launched["head_gemm"] == 2 * len(heads), launched
    fwd = 2 * flushes_of(row) if row.mode == "train" else 0
    bwd = 2 if row.merge is not None or row.mode == "eval" else 0
    assert launched.get("head_dgrad", 0) == fwd + bwd, launched


def flushes_of(row):
    """forward_heads calls of the row's one group: one per head_max hops"""
    hm = row.cls["head_max"]
    return (row.H + hm - 1) // hm


@rows("tiles", "bulk")
def test_row_tiles_and_the_bulk_tile_edge(monkeypatch, row):
    """Section 5: one and two 64-row tiles with a one-row last tile, both sides of the 64-sample switch and of
    colsum_acc's 128 rows; both sides of the one-launch 128 x 128 edge of lin_gemm."""
    check(monkeypatch, row)


# ---------------------------------------------------------------- 6. bf16 mode
@rows("bf16")
def test_bf16(monkeypatch, row):
    """tests/test_gpu_bf16.run at the row.  run() weights every hop; a gated row hands its own hop weights to the
    two places that read them, the oracle's step and the device's backward."""
    from oracle import ref_torch
    from rau_vqa_amd import model
    set_env(monkeypatch, row)
    if row.hop_w is not None:
        hop_w, real_step = hop_w_of(row), ref_torch.step

        def gated_step(*args, **kw):
            return real_step(*args[:7], hop_w, *args[8:], **kw)

        class Gated(model.RAU):
            def backward(self, _hop_w, **kw):
                return super().backward(hop_w, **kw)
        monkeypatch.setattr(ref_torch, "step", gated_step)
        monkeypatch.setattr(model, "RAU", Gated)
    print(f"rows[bf16] {row_id(row)}", end=": ")
    test_gpu_bf16.run(dims_of(row), SCALE, row.mode, lens=lens_of(row.B, row.T, row.TL))


# ---------------------------------------------------------------- 7. module level
@pytest.mark.parametrize("B", sorted(MODULE_B))
def test_module_level_feval(B):
    """The module-level weight gradients reduce over B rows: tn_splits with two splits and a partial last step, and
    the last B without a split."""
    test_gpu_positions.module_level_feval(dict(MODULE_DIMS, B=B), 4000 + B, f"rows[mod] B={B}")
