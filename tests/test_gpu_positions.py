"""Parity over the position count S: more of the kernel dispatch branches on S than on any other dimension.

Sp = (S + 3) & ~3 is the pitch of the device tensors; the step path hands Sp to the kernels as their S and the
logical count as SL (rau_ctx.hip: `S = ctx->Sp, SL = c.S`).  Pad columns [S, Sp) carry zero features, zero
attention and zero gradients.  The predicates, read off the code at this commit:

  predicate (file)                                   condition on the pitch
  conv_sample_ok (gemm_sample.hip)                   176 < Sp <= 208: one sample per 128 x 208 tile.  By default
      (RAU_CONV_SAMPLE = 12) for the attention dgrad, fused with (1 - I^2) and the bias row sums where
      conv_dz_fused_ok (gemm_conv.hip) says the same, and for the module-level feature-map gradient; the
      two forward convs take it only when the knob asks.  At Sp = 208 its LDS tile has no pad columns left.
  conv_wide_ok (conv_wide.hip)                       Sp == 196, rows % 64, reduction % 8: both forward convs, the
      samples of a launch in groups of four, the rest on the general tile (B = 6, train mode: both hops in one
      launch of 12, no rest; evaluate mode: 4 + 2; B = 66: one launch per hop, 64 + 2).
  dgrad_dma_ok (dgrad_dma.hip)                       Sp == 196, M % 128, A % 16, A >= 48, and not `light` (contexts
      above 64 samples): the attention dgrad's LDS-DMA tile.
  wgrad_dma_ok (wgrad_dma.hip)                       Sp == 196, both row counts % 128: both conv weight gradients
      where the operands are plain f32 (the i_embed one only behind the fused dZ).
  dgrad16_ok, wgrad16_ok (dgrad16.hip, wgrad16.hip)  Sp == 196, M % 128, A % 32 / M % 256, D % 256: bf16 mode.
  conv_wgrad_any (gemm_conv.hip)                     else: Sp % 28 == 0 -> 28-deep chunks, otherwise 32-deep with
      the last chunk zero-filled past Sp; bf16 mode always 32-deep.
  bf16 16-bit X / dZ storage (rau_ctx.hip)           Sp == S and conv_dz_fused_ok: S in {180, 184, .., 208};
      16-bit dS needs dgrad16_ok on top: S == 196 only.
  att_fwd_dma_ok, att_bwd_dma_sizes (kernels.hip)    Sp <= 256 (and A, M <= 512, LDS <= 96 KB): the LDS-DMA
      attention kernels of the fused family; RAU_ATT_DMA_OFF (read at every call) keeps the register-staged ones.
  k_att_fwd_fused, k_att_bwd_fused, k_att_score_part, k_att_da_part
                                                     `for (q0 = 0; q0 < Sp / 4; q0 += 64)`: a second trip above
      256 positions.
  attention family (rau_ctx.hip)                     split up to 64 samples, fused above; RAU_ATT_FUSED=1 keeps
      the fused one.
  skinny_dma.hip, gemm_lin.hip                       Linear products with K or N = S (attbymemory, feat_attprob).
  rau_create                                         refuses S above att_max_pitch (kernels.hip): 4096 positions in
      the split family, 900 in the fused one at A = 128 -- section 6 below.

The module-level calls pass T == nullptr to att_fwd_fused like the step path (hop_forward_chain), so they take
the same attention kernels; what differs there is one conv launch per hop over B samples, not one per hop group.

What each S is there for (CASES below adds the kernel every conv class takes at it): 36, 100 box-feature counts
(general tiles, 32-deep chunks with a 4-wide tail, Linear tails); 112 Sp % 28 == 0 away from 196; 176 last S below
the per-sample tile; 177 first S inside it (Sp = 180, three pad columns); 180 inside it, unpitched; 193, 195 every
`== 196` kernel on a pitched map; 196 control; 197, 200 Sp = 200 pitched and unpitched; 205, 208 Sp = 208: all 13
column blocks live, no LDS pad; 209 first S above the tile; 252 28-deep at 9 chunks; 253, 256 upper edge of the
LDS-DMA attention kernels; 257, 260 second trip of the q0 loop with one lane live; 400 a 20 x 20 map.

1. f32 step path against the fp64 autograd oracle: tests/test_gpu_parity.check's 1e-4 max-norm bar on every output
   and every layer's gradient, argmax exact on decided rows.  CASES says what each S is there for.
2. bf16 mode: tests/test_gpu_bf16.run and its derived bars, unchanged.
3. module-level feval against the step path on the same context (2e-5, tests/test_gpu_fuzz.py's bar).
4. (tests/test_gpu_regions.py: region counts at S = 100.)
6. rau_create's refusal above the attention kernels' LDS bound, on contexts that are never created.
7. From 400 positions to that bound (LARGE below, a table of its own: most of CASES' parametrisations do not apply
   up there): the checks of 1, 2 and 3 on contexts that are created and run, in both attention families and both
   modes.  tests/test_positions_host.py holds every label of the table, and every bound, to the launches in
   kernels.hip and to rau_create.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import util
from tests import test_gpu_bf16, test_gpu_parity

pytestmark = pytest.mark.gpu

# D = M = A = 128: the smallest widths that reach wgrad_dma (rows % 128), dgrad_dma (M % 128, A % 16, A >= 48),
# conv_wide (M % 64, D % 8) and the per-sample tile -- each at the right S only
F32 = dict(T=4, V=40, E=16, Rq=32, D=128, M=128, A=128, R=32, K=48, H=2)
B16 = dict(B=6, T=4, V=40, E=16, Rq=32, D=256, M=256, A=64, R=32, K=48, H=2)   # dgrad16's and wgrad16's shapes
SCALE = 0.2

# S: (pitch, forward convs, attention dgrad, conv weight gradients [f32, B = 6 / B = 66], why it is here).
# general = gemm_core.h's 128 x 128 flattened-column tile; sample = gemm_sample.hip; 28 / 32 = conv_wgrad's chunk.
# Train mode; in evaluate mode I is shared by the hops: the dgrad has no fused dZ and the i_embed weight gradient
# stages dI (1 - I^2) itself, which keeps it on conv_wgrad's chunks at every S (28-deep at 196).
# A comment for the next reader: the conv kernels have no profile class of their own to assert.
CASES = {
    36:  (36,  "general", "general", "32, 4-wide tail", "box features: general tiles, RAG Linear tails"),
    100: (100, "general", "general", "32, 4-wide tail", "box features"),
    112: (112, "general", "general", "28",              "Sp % 28 == 0 away from 196"),
    176: (176, "general", "general", "32, 16-wide tail", "last S below the per-sample tile"),
    177: (180, "general", "sample+dZ", "32, 20-wide tail", "first S inside it, pitched, three pad columns"),
    180: (180, "general", "sample+dZ", "32, 20-wide tail", "inside it, unpitched"),
    193: (196, "wide 12 / 64+2", "sample+dZ / dgrad_dma", "wgrad_dma", "every == 196 kernel, three pad columns"),
    195: (196, "wide 12 / 64+2", "sample+dZ / dgrad_dma", "wgrad_dma", "every == 196 kernel, one pad column"),
    196: (196, "wide 12 / 64+2", "sample+dZ / dgrad_dma", "wgrad_dma", "control"),
    197: (200, "general", "sample+dZ", "32, 8-wide tail", "Sp = 200, pitched"),
    200: (200, "general", "sample+dZ", "32, 8-wide tail", "Sp = 200, unpitched"),
    205: (208, "general", "sample+dZ", "32, 16-wide tail", "Sp = 208: 13 live column blocks, no LDS pad; pitched"),
    208: (208, "general", "sample+dZ", "32, 16-wide tail", "Sp = 208, unpitched"),
    209: (212, "general", "general", "32, 20-wide tail", "first S above the per-sample tile"),
    252: (252, "general", "general", "28, 9 chunks",    "28-deep at 9 chunks"),
    253: (256, "general", "general", "32",              "upper edge of the attention LDS-DMA kernels, pitched"),
    256: (256, "general", "general", "32",              "upper edge of the attention LDS-DMA kernels"),
    257: (260, "general", "general", "32, 4-wide tail", "S4 = 65: second trip of the q0 loop, one lane live"),
    260: (260, "general", "general", "32, 4-wide tail", "the same, unpitched"),
    400: (400, "general", "general", "32, 16-wide tail", "a 20 x 20 map, S4 = 100"),
}
S_LARGE_BATCH = (100, 193, 195, 196, 200, 256, 260)
S_FUSED = (100, 180, 195, 208, 256, 260, 400)
S_BF16 = (100, 180, 195, 200, 208, 256, 260)
S_MODULES = (100, 180, 200, 208, 256, 260, 400)

# From 400 positions to the bound (section 7).  Per row: the pitch; the trips of `for (q0 = 0; q0 < Sp / 4; q0 += 64)`
# and the lanes live in the last one; conv_wgrad's chunk depth in f32 (bf16 mode: always 32) and its chunks per
# sample; the pad columns; whether the pitch is the largest that rau_create accepts for the row's family, A and wave
# counts.  over: what replaces F32's dimensions; env: read when the context is created.
# tests/test_positions_host.py recomputes every label from S and holds `bound` to the launches' LDS requests.
Large = collections.namedtuple("Large", "sec S pitch trips lanes depth chunks pad bound why over env")


def _L(sec, S, pitch, trips, lanes, depth, chunks, pad, why, bound=False, over=None, env=None):
    return Large(sec, S, pitch, trips, lanes, depth, chunks, pad, bound, why, over or {}, env or {})


FUSED6 = {"RAU_ATT_FUSED": "1"}
FWD8 = {"RAU_ATT_WAVES_FWD": "8"}      # the evaluate-mode forward on 8 waves as well: the backward's term binds
TINY = dict(D=16, M=32, A=16)          # the B = 64 corner: memory and the oracle's time stay small
LARGE = [
    # split family, B = 6 (att_chunks = 8), train and evaluate mode
    _L("split", 512, 512, 2, 64, 32, 16, 0, "S4 = 128: two q0 trips that end exactly, two exact trips of `s += 256`"),
    _L("split", 513, 516, 3, 1, 32, 17, 3, "third trip with one lane live, pitched"),
    _L("split", 516, 516, 3, 1, 32, 17, 0, "the same, unpitched"),
    _L("split", 769, 772, 4, 1, 32, 25, 3, "fourth trip with one lane live, pitched"),
    _L("split", 772, 772, 4, 1, 32, 25, 0, "the same, unpitched"),
    _L("split", 896, 896, 4, 32, 28, 32, 0, "28-deep conv chunks at 32 chunks"),
    _L("split", 2048, 2048, 8, 64, 32, 64, 0, "32 KB of LDS, eight trips"),
    _L("split", 4088, 4088, 16, 62, 28, 146, 0, "28-deep chunks at 146 chunks; last trip with 62 lanes"),
    _L("split", 4093, 4096, 16, 64, 32, 128, 3, "three pad columns at the bound", bound=True),
    _L("split", 4096, 4096, 16, 64, 32, 128, 0, "the bound: a 65536-byte request", bound=True),
    # the largest context of the family: att_chunks = 8 still, att_split_part_floats at its maximum
    _L("split64", 4096, 4096, 16, 64, 32, 128, 0, "B = 64 at the bound", bound=True, over=TINY),
    # fused family, B = 66, train mode (8 forward waves) and evaluate mode (16: the term that binds)
    _L("fused", 512, 512, 2, 64, 32, 16, 0, "two exact trips; two exact trips of `s += NW * 64` at 8 waves"),
    _L("fused", 516, 516, 3, 1, 32, 17, 0, "third trip with one lane live"),
    _L("fused", 768, 768, 3, 64, 32, 24, 0, "three exact trips"),
    _L("fused", 772, 772, 4, 1, 32, 25, 0, "fourth trip with one lane live"),
    _L("fused", 896, 896, 4, 32, 28, 32, 0, "28-deep conv chunks at 32 chunks"),
    _L("fused", 897, 900, 4, 33, 32, 29, 3, "three pad columns at the bound", bound=True),
    _L("fused", 900, 900, 4, 33, 32, 29, 0, "the bound at A = 128: 18 Sp + 32 + A floats", bound=True),
    _L("fused", 889, 892, 4, 31, 32, 28, 3, "the bound at A = 256, pitched", bound=True, over=dict(A=256)),
    _L("fused", 892, 892, 4, 31, 32, 28, 0, "the bound at A = 256", bound=True, over=dict(A=256)),
    _L("fused", 904, 904, 4, 34, 32, 29, 0, "the bound at A = 16", bound=True, over=dict(A=16)),
    _L("fused", 960, 960, 4, 48, 32, 30, 0, "the backward's bound, 17 Sp + 16 floats, with 8 forward waves in "
       "both modes", bound=True, env=FWD8),
    # fused family at B = 6, the forward's class asserted from the profile
    _L("fused6", 516, 516, 3, 1, 32, 17, 0, "register-staged pair, third trip", env=FUSED6),
    _L("fused6", 772, 772, 4, 1, 32, 25, 0, "fourth trip", env=FUSED6),
    _L("fused6", 900, 900, 4, 33, 32, 29, 0, "the bound", bound=True, env=FUSED6),
]
# bf16 mode (B16: A = 64, B = 6, split family) and the module-level calls (F32, B = 6): rows of S alone
S_BF16_LARGE = [(516, "train"), (900, "train"), (4096, "train"), (900, "eval"), (4096, "eval")]
S_MODULES_LARGE = (516, 900, 4096)


def large_rows(sec):
    return [r for r in LARGE if r.sec == sec]


def large_id(r):
    return "-".join([str(r.S)] + [f"{k}{v}" for k, v in sorted(r.over.items())] + sorted(r.env))


ATT_ENV = ("RAU_ATT_SPLIT", "RAU_ATT_FUSED", "RAU_ATT_DMA_OFF", "RAU_ATT_CHUNKS")
WAVE_ENV = ("RAU_ATT_WAVES_FWD", "RAU_ATT_WAVES_BWD")


def test_the_case_table_states_the_pitch():
    assert all(row[0] == (S + 3) & ~3 for S, row in CASES.items())


# ---------------------------------------------------------------- 1. f32 step path
_REFERENCES = {}


def check(monkeypatch, S, B, mode, env=None, prof=False, over=None):
    """tests/test_gpu_parity.check at (S, B); the fp64 reference of a problem is computed once for the families
    that run it.  prof: run the context with its profile on (every launch is then bracketed by two events:
    only where a class is asserted, the rest runs as a training step does) and return what the step launched, by class.
    over: dimensions that replace F32's (tests/test_gpu_widths.py sweeps the widths through this)."""
    from oracle import ref_torch
    from rau_vqa_amd import model
    for k in ATT_ENV + WAVE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)               # read when the context is created / at every launch
    real_step = ref_torch.step
    dims = dict(F32, B=B, S=S, **(over or {}))
    key = (mode,) + tuple(sorted(dims.items()))

    def step_once(*args, **kw):
        if key not in _REFERENCES:
            _REFERENCES[key] = real_step(*args, **kw)
        return _REFERENCES[key]
    launched = {}

    class Profiled(model.RAU):
        def __init__(self, cfg):
            super().__init__(cfg)
            self.prof_enable()

        def close(self):
            self.sync()
            launched.update({k: v["launches"] for k, v in self.prof().items()})
            super().close()
    monkeypatch.setattr(ref_torch, "step", step_once)
    if prof:
        monkeypatch.setattr(model, "RAU", Profiled)
    sh = util.shapes(dims)
    errs = test_gpu_parity.check(sh, scale=SCALE, torch_oracle=True, mode=mode)
    what = "".join(f" {k}={v}" for k, v in sorted((over or {}).items()))
    print(f"S={S} B={B}{what} {mode}: largest error / bar {max(errs.values()) / test_gpu_parity.TOL:.3f}")
    return launched


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("S", sorted(CASES))
def test_small_batch(monkeypatch, S, mode):
    """B = 6: conv_wide on 12 samples (train: the two hops in one launch) or on four plus two on the general tile
    (evaluate); split attention family, `light` dgrad."""
    check(monkeypatch, S, 6, mode)


@pytest.mark.parametrize("S", S_LARGE_BATCH)
def test_large_batch(monkeypatch, S):
    """B = 66 = 64 + 2: the large-batch policies, the fused attention family, dgrad_dma."""
    check(monkeypatch, S, 66, "train")


@pytest.mark.parametrize("dma_off", [False, True], ids=["FUSED", "FUSED DMA_OFF"])
@pytest.mark.parametrize("S", S_FUSED)
def test_fused_family_at_a_small_batch(monkeypatch, S, dma_off):
    """Each kernel of the fused family at each S class: the LDS-DMA pair up to 256 positions, the register-staged
    pair above them or with RAU_ATT_DMA_OFF."""
    env = {"RAU_ATT_FUSED": "1"}
    if dma_off:
        env["RAU_ATT_DMA_OFF"] = "1"
    launched = check(monkeypatch, S, 6, "train", env, prof=True)
    regs = dma_off or CASES[S][0] > 256
    fwd = {k: v for k, v in launched.items() if k.startswith("att_fwd")}
    assert fwd == {"att_fwd_fused_regs" if regs else "att_fwd_fused": F32["H"]}, launched


# ---------------------------------------------------------------- 2. bf16 mode
@pytest.mark.parametrize("S,mode", [(S, "train") for S in S_BF16] + [(180, "eval"), (260, "eval")])
def test_bf16(S, mode):
    """180, 200, 208: 16-bit dZ / X storage away from 196 (the per-sample tile's bf16 epilogue, conv_wgrad's
    stored-bf16 loaders with a zero-filled last chunk); 195: dgrad16 on a pitched map, f32 storage."""
    test_gpu_bf16.run(dict(B16, S=S), SCALE, mode)


# ---------------------------------------------------------------- 3. module-level calls
TOL_MODULES = 2e-5     # tests/test_gpu_fuzz.py::test_random_shapes_module_level_feval's bar


def module_level_feval(dims, seed, label):
    """tests/test_gpu_fuzz.py::test_random_shapes_module_level_feval's body and bar at `dims`."""
    import torch
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import make_model, cuda
    sh = util.shapes(dims)
    lens = np.random.default_rng(seed).integers(0, dims["T"] + 1, dims["B"]).astype(np.int32)
    lens[0] = dims["T"]
    batch, params, masks = util.make_problem(sh, lens=lens, scale=SCALE)
    hop_w = np.full(sh.H, 1.0, np.float32)
    m = make_model(sh, params, masks)
    m.zero_grads()
    modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32),
                  cuda(batch["lens"], torch.int32), cuda(batch["labels"], torch.int32), hop_w)
    m.sync()
    g_mod = m.get_grads()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.zero_grads()
    m.forward()
    m.backward(hop_w)
    g_step = m.get_grads()
    m.close()
    errs = {k: util.rel_err(g_mod[k], g_step[k]) for k in g_step}
    print(f"{label}: largest error / bar {max(errs.values()) / TOL_MODULES:.3f}")
    for k in g_step:
        assert errs[k] < TOL_MODULES, (k, dims)


@pytest.mark.parametrize("S", S_MODULES)
def test_module_level_feval(S):
    module_level_feval(dict(F32, B=6, S=S), 2000 + S, f"S={S}")


# ---------------------------------------------------------------- 6. the upper end
@pytest.mark.parametrize("over,S,refused,family", [
    (dict(B=6), 4096, False, None),                    # split family: 4 Sp floats of LDS = 64 KB at 4096
    (dict(B=6), 4097, True, b"4096 positions at which the split"),
    (dict(B=66), 897, False, None),                    # fused, 16 forward waves: 18 Sp + 32 + A floats; pitch 900
    (dict(B=66), 901, True, b"900 positions at which the fused"),
    (dict(B=66, A=256), 893, True, b"892 positions at which the fused"),
    (dict(B=66, dtype=1), 901, True, b"900 positions at which the fused"),
    (dict(B=66), 900, False, None),                    # the bounds that section 7 runs
    (dict(B=66, A=256), 892, False, None),
    (dict(B=66, A=16), 904, False, None),
    (dict(B=66, A=16), 905, True, b"904 positions at which the fused"),
    (dict(B=66, env=FWD8), 960, False, None),          # `env`: set when rau_create reads its policy, not a dimension
    (dict(B=66, env=FWD8), 961, True, b"960 positions at which the fused"),
])
def test_create_refuses_what_an_attention_kernel_cannot_launch(monkeypatch, over, S, refused, family):
    """By reading (kernels.hip att_max_pitch), nothing is launched: the configuration checks of rau_create come
    before it touches the device, so an accepted S is told apart by getting past them -- here to the device
    check, which device_id = -1 fails."""
    from rau_vqa_amd import _lib
    over = dict(over)
    for k in ATT_ENV + WAVE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in over.pop("env", {}).items():
        monkeypatch.setenv(k, v)
    lib = _lib.lib()
    cfg = _lib.RauConfig()
    lib.rau_default_config(C.byref(cfg))
    for k, v in dict(F32, S=S, device_id=-1, **over).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert lib.rau_create(C.byref(cfg), C.byref(h)) == -1      # RAU_ERR_INVALID either way
    assert not h.value
    msg = lib.rau_last_error()
    if refused:
        assert family in msg and b"64 KB" in msg, msg
    else:
        assert b"device_id" in msg, msg


# ---------------------------------------------------------------- 7. from 400 positions to the bound
def clear_env(monkeypatch):
    for k in ATT_ENV + WAVE_ENV:
        monkeypatch.delenv(k, raising=False)


def test_the_large_table_states_the_pitch():
    assert all(r.pitch == (r.S + 3) & ~3 and 400 < r.S for r in LARGE)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("row", large_rows("split") + large_rows("split64"), ids=large_id)
def test_split_family_to_its_bound(monkeypatch, row, mode):
    """B = 6, and B = 64 at the bound: k_att_score_part and k_att_da_part with 4 Sp floats of LDS, up to the 64 KB
    that a launch gets; up to 16 trips of the q0 loop."""
    check(monkeypatch, row.S, 64 if row.sec == "split64" else 6, mode, row.env, over=row.over)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("row", large_rows("fused"), ids=large_id)
def test_fused_family_to_its_bound(monkeypatch, row, mode):
    """B = 66.  Evaluate mode runs the forward on 16 waves: (16 + 2) Sp + 32 + A floats, the request that sets the
    bound; under RAU_ATT_WAVES_FWD=8 the 16-wave backward sets it."""
    check(monkeypatch, row.S, 66, mode, row.env, over=row.over)


@pytest.mark.parametrize("row", large_rows("fused6"), ids=large_id)
def test_fused_family_at_a_small_batch_to_its_bound(monkeypatch, row):
    launched = check(monkeypatch, row.S, 6, "train", row.env, prof=True)
    fwd = {k: v for k, v in launched.items() if k.startswith("att_fwd")}
    assert fwd == {"att_fwd_fused_regs": F32["H"]}, launched


@pytest.mark.parametrize("S,mode", S_BF16_LARGE)
def test_bf16_to_the_bound(monkeypatch, S, mode):
    """conv_wgrad's 32-deep bf16 chunks up to 128 per sample, the split attention family on bf16-mode operands.
    tests/test_positions_host.py holds the emulation alone to the same bars at these S."""
    clear_env(monkeypatch)
    test_gpu_bf16.run(dict(B16, S=S), SCALE, mode)


@pytest.mark.parametrize("S", S_MODULES_LARGE)
def test_module_level_feval_to_the_bound(monkeypatch, S):
    clear_env(monkeypatch)
    module_level_feval(dict(F32, B=6, S=S), 2000 + S, f"S={S}")
