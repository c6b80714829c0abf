"""Parity over the channel widths D, M, A and the batch count at S = 196: the other half of the kernel dispatch.

tests/test_gpu_positions.py sweeps the position count; the kernels compiled for a 14 x 14 map branch as hard on
the widths and on the number of samples a launch gets.  The predicates, read off the code at this commit
(tests/test_widths_host.py restates them and holds CASES below to them):

  predicate (file)                  condition at S = 196
  conv_wide_ok (conv_wide.hip)      rows % 64, reduction % 8 and >= 16 (two K-steps): both forward convs in exact
      f32, i_embed with (rows, reduction) = (M, D), ifeatproj with (A, M).  A launch of n samples puts n & ~3 on
      the wide tile and the rest on the general one; n < 4: no wide launch.  n = H B where a context of up to 64
      samples runs the hops as one launch group (train mode), B in evaluate mode (I is shared by the hops) and
      above 64 samples (H = 2: one group per hop).
  conv_sample_ok (gemm_sample.hip)  mask 12: the attention dgrad (4) and the module-level feature-map gradient (8)
      at every width that is a multiple of 4; partial 128-row tiles where M % 128 != 0.
  conv_dz_fused_ok (gemm_conv.hip)  M % 4: always at S = 196; the train-mode dgrad applies (1 - I^2) itself.
  dgrad_dma_ok (dgrad_dma.hip)      M % 128, A % 16, A >= 48 (a ring of three 16-row stages), and not `light`:
      `light` (rau_ctx.h chain_bound) is evaluate mode, bf16 mode or a context of up to 64 samples.
  wgrad_dma_ok (wgrad_dma.hip)      both row counts % 128, plain f32 operands: the att_i gradient (A, M) in both
      modes, the i_embed one (M, D) in train mode only (evaluate mode stages dI (1 - I^2) itself: conv_wgrad's
      28-deep chunks).  Split count min(512 / tiles, samples); two wave groups per workgroup up to 8 tiles.
  dgrad16_ok (dgrad16.hip)          bf16 mode: M % 128, A % 32, A >= 32.
  wgrad16_ok (wgrad16.hip)          bf16 mode: M % 128, D % 256 (else conv_wgrad's stored-bf16 loaders).
  16-bit storage (rau_ctx.hip)      bf16 mode, train: X' and dZ as bf16 at every width (conv_dz_fused_ok); dS as
      bf16 where dgrad16_ok and the LDS-DMA attention backward applies (A, M <= 512), and then only in the
      fused family -- at B = 6 the split family writes f32 dS, so those rows set RAU_ATT_FUSED.
  attention family (rau_ctx.hip)    split up to 64 samples, fused above (RAU_ATT_FUSED keeps it below, RAU_ATT_SPLIT
      the split one above); row chunks per sample of the split kernels (att_chunks): 8 up to 64 samples, else 4.
  att_fwd_dma_ok, att_bwd_dma_sizes (kernels.hip)
                                    A <= 512 and M <= 512 (one lane per row a wave owns: 64 x 8 waves).  Above
      that the register-staged k_att_fwd_fused / k_att_bwd_fused run: by reading they have no width limit of
      their own (rows are strided over the waves, u of A floats sits behind the [NW + 2][S] LDS block that
      att_max_pitch already counts), and the rows A = 516, 640 and M = 516, 640 below hold them to that.
  skinny_dma.hip stage_depth, ragged
                                    a Linear product of reduction length k: 32-deep stages where `deep`
      (= `light`) and k % 64 == 0; else 16-deep, ragged unless k % 32 == 0; [K][N] weights (the input-gradient
      products) are ragged as well where N % 64 != 0.  Every class is reachable through rau_create's rules
      (widths are multiples of 4, which is all the ragged kernels ask for).

Section 5 (module level): tests/test_gpu_positions.module_level_feval at one row per conv class of the table --
the control (conv_wide 4 + 2 per hop against the step's 12; wgrad_dma with 6 samples per launch against 12),
D = 16 (the two-K-step wide tile with a general-tile tail), M = A = 192 (three row tiles; both weight gradients on
conv_wgrad's chunks), M = 132 (general forward tiles, a partial row tile of the per-sample dgrad) and M = 384
(non-square wgrad_dma grids whose split count is the sample count, 6 against 12).

Section 6 (Linear reduction classes).  The Linear products, as (form, N, reduction) of gemm_lin.hip's
gemm_nt / gemm_nn(M = rows, N, K) calls in rau_ctx.hip -- LIN_CALLS below; every one takes the context's
LinMode, so `deep` is chain_bound(): true for every B = 6 row and in bf16 mode, false for the f32 B = 66 row.
With R = Rq = K = w:  w = 64: every reduction over R, Rq, 4R, 4Rq or K is % 64 (32-deep where deep) and every
[K][N] weight has N % 64 == 0;  w = 96: 96 is % 32 only (16-deep, not ragged), 4w = 384 is % 64 again, N = 96
makes the [K][N] products ragged;  w = 100: 100 and 400 are ragged in both forms.  M = A = 128 and S = 196, E = 16
add a % 64 and two ragged reductions at every w.
"""
from collections import namedtuple

import pytest

from tests import test_gpu_bf16, test_gpu_positions

pytestmark = pytest.mark.gpu

S = 196
H = test_gpu_positions.F32["H"]
SCALE = test_gpu_positions.SCALE

# sec: the section that runs the row.  fwd: i_embed forward, ifeatproj forward.  wgrad: att_i, i_embed.
#   forward    wide = conv_wide alone, wide+tail = conv_wide + the rest on the general tile, general = gemm_core.h's
#              128 x 128 flattened-column tile; bf16 mode: b16 = that tile on stored-bf16 operands, bf16 = on f32
#              operands rounded while staged
#   dgrad      sample+dZ = gemm_sample.hip with the fused (1 - I^2) epilogue, sample = without (evaluate mode),
#              sample+dZ16 = the same with a bf16 dZ, dgrad16 / dgrad16+dS16 = dgrad16.hip on f32 / bf16 dS
#   wgrad      dma = wgrad_dma.hip, 28 = conv_wgrad's 28-deep chunks (28dtanh: staging dI (1 - I^2)),
#              32bf16 / 32bf16dtanh = 32-deep chunks rounding f32 operands, ds16 = bf16 dS beside f32 I,
#              b16 = both operands stored bf16, wgrad16 = wgrad16.hip
#   att        split, fused (LDS-DMA pair), fused_regs (register-staged pair)
Row = namedtuple("Row", "sec D M A B dtype mode fwd dgrad wgrad att why env over", defaults=({}, {}))
FUSED = {"RAU_ATT_FUSED": "1"}

CASES = [
    # ---- 1. f32, B = 6: 12 samples per forward launch in train mode, 6 (4 + 2) in evaluate mode; `light`
    Row("small", 128, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split", "control"),
    Row("small", 16, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma 28", "split",
        "conv_wide's minimum: two K-steps, the loop between prologue and tail never runs"),
    Row("small", 8, 128, 128, 6, "f32", "train", "general wide", "sample+dZ", "dma 28", "split",
        "one K-step: below conv_wide's minimum"),
    Row("small", 24, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma 28", "split",
        "an odd number of K-steps (3): one trip of the loop, the ring's third stage"),
    Row("small", 72, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma 28", "split",
        "nine K-steps; the i_embed gradient fails wgrad_dma (D) while the att_i one takes it"),
    Row("small", 132, 128, 128, 6, "f32", "train", "general wide", "sample+dZ", "dma 28", "split",
        "i_embed reduction % 4 but not % 8 with rows % 64: conv_wide refused on the reduction alone"),
    Row("small", 128, 132, 128, 6, "f32", "train", "general general", "sample+dZ", "28 28", "split",
        "ifeatproj reduction % 4 but not % 8 with rows % 64; a 4-row second tile of the per-sample dgrad"),
    Row("small", 128, 96, 128, 6, "f32", "train", "general wide", "sample+dZ", "28 28", "split",
        "i_embed rows % 64 != 0 (and % 32 == 0) beside an eligible ifeatproj"),
    Row("small", 128, 128, 96, 6, "f32", "train", "wide general", "sample+dZ", "28 dma", "split",
        "ifeatproj rows % 64 != 0; the att_i gradient fails wgrad_dma (A) while the i_embed one takes it"),
    Row("small", 128, 192, 192, 6, "f32", "train", "wide wide", "sample+dZ", "28 28", "split",
        "three row tiles of conv_wide in both convs; a half second tile of the per-sample dgrad"),
    Row("small", 256, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "a 1 x 2 tile grid of the i_embed wgrad_dma, 12 splits"),
    Row("small", 128, 384, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "1 x 3 and 3 x 1 wgrad_dma grids; three full row tiles of the per-sample dgrad"),
    Row("small", 128, 128, 32, 6, "f32", "train", "wide general", "sample+dZ", "28 dma", "split",
        "per-sample dgrad at one 32-deep K-step"),
    Row("small", 128, 128, 48, 6, "f32", "train", "wide general", "sample+dZ", "28 dma", "split",
        "per-sample dgrad whose reduction ends inside a K-step"),
    Row("small", 128, 128, 72, 6, "f32", "train", "wide general", "sample+dZ", "28 dma", "split",
        "per-sample dgrad, A % 16 != 0"),
    Row("small", 128, 128, 80, 6, "f32", "train", "wide general", "sample+dZ", "28 dma", "split",
        "per-sample dgrad, A % 16 == 0 and % 32 != 0"),
    Row("small", 128, 128, 640, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "the split attention family above 512 rows of P (it has no DMA form: no width rule)"),
    Row("small", 128, 640, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "the split attention family above 512 rows of I"),
    # evaluate mode: I shared, no fused dZ, conv_embed_wgrad stages dI (1 - I^2) itself
    Row("small", 128, 128, 128, 6, "f32", "eval", "wide+tail wide+tail", "sample", "dma 28dtanh", "split", "control"),
    Row("small", 16, 128, 128, 6, "f32", "eval", "wide+tail wide+tail", "sample", "dma 28dtanh", "split",
        "two K-steps with a tail on the general tile at K = 16"),
    Row("small", 132, 128, 128, 6, "f32", "eval", "general wide+tail", "sample", "dma 28dtanh", "split",
        "general i_embed tile over six samples"),
    Row("small", 128, 132, 128, 6, "f32", "eval", "general general", "sample", "28 28dtanh", "split",
        "the plain per-sample dgrad epilogue on a 4-row second tile; the DTANH loader at M % 128 != 0"),
    Row("small", 128, 192, 192, 6, "f32", "eval", "wide+tail wide+tail", "sample", "28 28dtanh", "split",
        "three row tiles with a tail"),
    Row("small", 128, 128, 96, 6, "f32", "eval", "wide+tail general", "sample", "28 28dtanh", "split",
        "neither weight gradient on wgrad_dma"),
    Row("small", 128, 384, 128, 6, "f32", "eval", "wide+tail wide+tail", "sample", "dma 28dtanh", "split",
        "a 1 x 3 wgrad_dma grid with six samples per launch"),
    # ---- 2. f32, B = 66: one launch per hop (64 + 2), fused family, dgrad_dma eligible
    Row("large", 128, 128, 128, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused", "control"),
    Row("large", 128, 128, 32, 66, "f32", "train", "wide+tail general", "sample+dZ", "28 dma", "fused",
        "below dgrad_dma's ring depth (two stages)"),
    Row("large", 128, 128, 48, 66, "f32", "train", "wide+tail general", "dgrad_dma", "28 dma", "fused",
        "dgrad_dma's minimum: three stages, the ring filled once"),
    Row("large", 128, 128, 72, 66, "f32", "train", "wide+tail general", "sample+dZ", "28 dma", "fused",
        "A % 16 != 0 above the minimum"),
    Row("large", 128, 128, 80, 66, "f32", "train", "wide+tail general", "dgrad_dma", "28 dma", "fused",
        "an odd stage count (5)"),
    Row("large", 128, 192, 128, 66, "f32", "train", "wide+tail wide+tail", "sample+dZ", "28 28", "fused",
        "M % 128 != 0 with everything else eligible"),
    Row("large", 128, 384, 128, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "three row tiles of dgrad_dma; 1 x 3 and 3 x 1 wgrad_dma grids"),
    Row("large", 256, 128, 128, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "M = 128 with D = 256: a 1 x 2 grid"),
    Row("large", 128, 384, 384, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "a 3 x 3 grid: 512 / 9 = 56 splits, fewer than samples, one wave group; 24 dgrad stages"),
    Row("large", 128, 512, 256, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "a 2 x 4 grid: the last tile count (8) with two wave groups, 64 splits; M = 512, the edge of the LDS-DMA pair"),
    Row("large", 128, 128, 512, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "the LDS-DMA attention pair at its edge: 64 rows per wave, one per lane"),
    Row("large", 128, 128, 516, 66, "f32", "train", "wide+tail general", "sample+dZ", "28 dma", "fused_regs",
        "first A above the edge"),
    Row("large", 128, 128, 640, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused_regs",
        "a clean % 128 A above the edge: 40 dgrad stages, a 5 x 1 grid"),
    Row("large", 128, 516, 128, 66, "f32", "train", "general general", "sample+dZ", "28 28", "fused_regs",
        "first M above the edge"),
    Row("large", 128, 640, 128, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused_regs",
        "a clean % 128 M above the edge: five row tiles everywhere"),
    # the width edge again in the fused family of a small batch
    Row("fused6", 128, 128, 512, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "fused", "the edge", FUSED),
    Row("fused6", 128, 128, 516, 6, "f32", "train", "wide general", "sample+dZ", "28 dma", "fused_regs", "A above", FUSED),
    Row("fused6", 128, 128, 640, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "fused_regs", "A above, % 128", FUSED),
    Row("fused6", 128, 516, 128, 6, "f32", "train", "general general", "sample+dZ", "28 28", "fused_regs", "M above", FUSED),
    Row("fused6", 128, 640, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "fused_regs", "M above, % 128", FUSED),
    # ---- 3. the sample count of a launch, control widths
    Row("batch", 128, 128, 128, 1, "f32", "train", "general general", "sample+dZ", "dma dma", "split",
        "2 samples per launch: no wide launch in train mode"),
    Row("batch", 128, 128, 128, 3, "f32", "train", "wide+tail wide+tail", "sample+dZ", "dma dma", "split", "6 = 4 + 2"),
    Row("batch", 128, 128, 128, 4, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split", "8: no tail"),
    Row("batch", 128, 128, 128, 5, "f32", "train", "wide+tail wide+tail", "sample+dZ", "dma dma", "split", "10 = 8 + 2"),
    Row("batch", 128, 128, 128, 7, "f32", "train", "wide+tail wide+tail", "sample+dZ", "dma dma", "split", "14 = 12 + 2"),
    Row("batch", 128, 128, 128, 3, "f32", "eval", "general general", "sample", "dma 28dtanh", "split",
        "3 samples: no wide launch"),
    Row("batch", 128, 128, 128, 4, "f32", "eval", "wide wide", "sample", "dma 28dtanh", "split", "4: one group, no tail"),
    Row("batch", 128, 128, 128, 5, "f32", "eval", "wide+tail wide+tail", "sample", "dma 28dtanh", "split", "remainder 1"),
    Row("batch", 128, 128, 128, 7, "f32", "eval", "wide+tail wide+tail", "sample", "dma 28dtanh", "split", "remainder 3"),
    Row("batch", 128, 128, 128, 64, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "last batch of the split family, `light`, 8 chunks, one launch group of 128"),
    Row("batch", 128, 128, 128, 65, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "first batch of the fused family, dgrad_dma, a group per hop: 64 + 1, remainder 1 in train mode"),
    Row("batch", 128, 128, 128, 65, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "split",
        "the split family above 64 samples: 4 row chunks per sample instead of 8", {"RAU_ATT_SPLIT": "1"}),
    Row("batch", 128, 128, 128, 67, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "64 + 3: remainder 3 in train mode"),
    # ---- 4. bf16 mode, B = 6
    Row("bf16", 256, 256, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split", "control"),
    Row("bf16", 256, 256, 32, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split",
        "dgrad16's minimum: one K-step"),
    Row("bf16", 256, 256, 48, 6, "bf16", "train", "b16 b16", "sample+dZ16", "32bf16 wgrad16", "split",
        "A % 32 != 0: wgrad16 without dgrad16"),
    Row("bf16", 256, 256, 96, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split",
        "an odd number of K-steps (3)"),
    Row("bf16", 256, 128, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split", "one dZ tile"),
    Row("bf16", 256, 384, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split", "three dZ tiles"),
    Row("bf16", 512, 256, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split", "two X tiles"),
    Row("bf16", 384, 256, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 b16", "split",
        "D % 256 != 0: dgrad16 without wgrad16, conv_wgrad's stored-bf16 loaders"),
    Row("bf16", 256, 192, 64, 6, "bf16", "train", "b16 b16", "sample+dZ16", "32bf16 b16", "split",
        "M % 128 != 0: neither kernel, no 16-bit dS"),
    Row("bf16", 256, 192, 64, 6, "bf16", "eval", "bf16 bf16", "sample", "32bf16 32bf16dtanh", "split",
        "the same row in evaluate mode: f32 storage, every operand rounded while staged"),
    Row("bf16", 256, 256, 64, 6, "bf16", "train", "b16 b16", "dgrad16+dS16", "ds16 wgrad16", "fused",
        "16-bit dS (fused family): the LDS-DMA backward's bf16 epilogue into dgrad16 and conv_wgrad", FUSED),
    Row("bf16", 256, 256, 32, 6, "bf16", "train", "b16 b16", "dgrad16+dS16", "ds16 wgrad16", "fused",
        "16-bit dS at one K-step", FUSED),
    Row("bf16", 256, 256, 640, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "fused_regs",
        "dgrad16_ok above the attention width edge: no 16-bit dS, the register-staged backward", FUSED),
    # ---- 6. Linear reduction classes (module docstring)
    Row("lin", 128, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "% 64: 32-deep stages", {}, dict(R=64, Rq=64, K=64)),
    Row("lin", 128, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "% 32 only: 16-deep, not ragged; N = 96 ragged", {}, dict(R=96, Rq=96, K=96)),
    Row("lin", 128, 128, 128, 6, "f32", "train", "wide wide", "sample+dZ", "dma dma", "split",
        "ragged in both forms", {}, dict(R=100, Rq=100, K=100)),
    Row("lin", 128, 128, 128, 66, "f32", "train", "wide+tail wide+tail", "dgrad_dma", "dma dma", "fused",
        "not deep: % 64 on 16-deep stages", {}, dict(R=64, Rq=64, K=64)),
    Row("lin", 256, 256, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split",
        "% 64, bf16 products", {}, dict(R=64, Rq=64, K=64)),
    Row("lin", 256, 256, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split",
        "% 32 only, bf16 products", {}, dict(R=96, Rq=96, K=96)),
    Row("lin", 256, 256, 64, 6, "bf16", "train", "b16 b16", "dgrad16", "32bf16 wgrad16", "split",
        "ragged, bf16 products", {}, dict(R=100, Rq=100, K=100)),
]

# 5. module level: (D, M, A) of "small" train rows, one per conv class (module docstring)
MODULE_WIDTHS = [(128, 128, 128), (16, 128, 128), (128, 192, 192), (128, 132, 128), (128, 384, 128)]

# The Linear products: (layer, form, N, reduction) in the model's dimensions (Q = 4 Rq); nt = x W^T on [N][K]
# weights (forward), nn = dy W on [K][N] weights (input gradient).
LIN_CALLS = [
    ("l1_i2h", "nt", "4*Rq", "E"), ("l*_h2h, l2_i2h", "nt", "4*Rq", "Rq"), ("q_proj", "nt", "M", "4*Rq"),
    ("h_proj", "nt", "M", "R"), ("att_mem", "nt", "S", "R"), ("lstm_h2h", "nt", "4*R", "R"),
    ("att_q", "nt", "A", "M"), ("feat_attprob", "nt", "M", "S"), ("lstm_i2h", "nt", "4*R", "M"),
    ("lstm_out", "nt", "M", "R"), ("cls", "nt", "K", "M"),
    ("cls", "nn", "M", "K"), ("lstm_out", "nn", "R", "M"), ("lstm_i2h", "nn", "M", "4*R"),
    ("lstm_h2h", "nn", "R", "4*R"), ("feat_attprob", "nn", "S", "M"), ("att_mem", "nn", "R", "S"),
    ("att_q", "nn", "M", "A"), ("h_proj", "nn", "R", "M"), ("q_proj", "nn", "4*Rq", "M"),
    ("l*_h2h, l2_i2h", "nn", "Rq", "4*Rq"), ("l1_i2h", "nn", "E", "4*Rq"),
]
# reduction length -> stage form where deep ("32", "16" = 16-deep and not ragged, "rag"), and whether a [K][N]
# weight of that N keeps the launch off the ragged kernels
LIN_DEPTH = {16: "rag", 64: "32", 96: "16", 100: "rag", 128: "32", 196: "rag", 256: "32", 384: "32", 400: "rag"}
LIN_N_OK = {16: False, 64: True, 96: False, 100: False, 128: True, 196: False, 256: True, 384: True, 400: False}


def dims_of(row):
    base = test_gpu_positions.B16 if row.dtype == "bf16" else test_gpu_positions.F32
    return dict(base, B=row.B, S=S, D=row.D, M=row.M, A=row.A, **row.over)


def row_id(row):
    extra = "".join(f"-{k}{v}" for k, v in sorted(row.over.items())) + "".join("-" + k[8:] for k in sorted(row.env))
    return f"D{row.D}-M{row.M}-A{row.A}-B{row.B}-{row.dtype}-{row.mode}{extra}"


def rows(*secs):
    sel = [r for r in CASES if r.sec in secs]
    return pytest.mark.parametrize("row", sel, ids=[row_id(r) for r in sel])


def run_f32(monkeypatch, row, prof=False):
    over = dict(D=row.D, M=row.M, A=row.A, **row.over)
    return test_gpu_positions.check(monkeypatch, S, row.B, row.mode, row.env, prof=prof, over=over)


def forward_attention_classes(launched):
    return {k: v for k, v in launched.items() if k.startswith("att_fwd")}


# ---------------------------------------------------------------- 1. - 3., 6.: f32 against the fp64 oracle
@rows("small")
def test_small_batch(monkeypatch, row):
    """B = 6: split attention family, `light` dgrad; conv_wide, wgrad_dma and the per-sample dgrad tile over
    D, M, A in train mode, and the rows whose dispatch differs in evaluate mode."""
    run_f32(monkeypatch, row)


@rows("large")
def test_large_batch(monkeypatch, row):
    """B = 66: dgrad_dma's A and M rows, the non-square wgrad_dma grids, the attention width edge -- where the
    forward must have launched the class the table states."""
    launched = run_f32(monkeypatch, row, prof=True)
    want = {"fused": "att_fwd_fused", "fused_regs": "att_fwd_fused_regs"}[row.att]
    assert forward_attention_classes(launched) == {want: H}, launched


@rows("fused6")
def test_width_edge_in_the_fused_family_at_a_small_batch(monkeypatch, row):
    launched = run_f32(monkeypatch, row, prof=True)
    want = {"fused": "att_fwd_fused", "fused_regs": "att_fwd_fused_regs"}[row.att]
    assert forward_attention_classes(launched) == {want: H}, launched


@rows("batch")
def test_samples_per_launch(monkeypatch, row):
    """The remainder classes of conv_wide (n & ~3 wide, the rest general; n < 4; n % 4 == 0) and both sides of
    the 64-sample edge, where the family, `light` and the chunk count change together."""
    launched = run_f32(monkeypatch, row, prof=row.B >= 64)
    if row.B >= 64:
        want = {"split": "att_fwd_split", "fused": "att_fwd_fused"}[row.att]
        assert forward_attention_classes(launched) == {want: H}, launched
        assert ("att_bwd_split" in launched) == (row.att == "split"), launched


@rows("lin")
def test_linear_reduction_classes(monkeypatch, row):
    """Recurrent widths that put every Linear product's reduction in each skinny_dma class (section 6)."""
    if row.dtype == "bf16":
        run_bf16(monkeypatch, row)
    else:
        run_f32(monkeypatch, row)


# ---------------------------------------------------------------- 4. bf16 mode
def run_bf16(monkeypatch, row):
    for k in test_gpu_positions.ATT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)               # read when the context is created
    print(row_id(row), end=": ")
    test_gpu_bf16.run(dims_of(row), SCALE, row.mode)


@rows("bf16")
def test_bf16(monkeypatch, row):
    """dgrad16 / wgrad16 over their tile counts and K-steps, each alone, neither, and the 16-bit dS storage."""
    run_bf16(monkeypatch, row)


# ---------------------------------------------------------------- 5. module-level calls
@pytest.mark.parametrize("D,M,A", MODULE_WIDTHS)
def test_module_level_feval(D, M, A):
    dims = dict(test_gpu_positions.F32, B=6, S=S, D=D, M=M, A=A)
    test_gpu_positions.module_level_feval(dims, 3000 + D + M + A, f"D={D} M={M} A={A}")
