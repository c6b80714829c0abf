"""tests/test_gpu_positions.py's LARGE table (400 positions to the bound) held to the code, without a device.

The LDS request of every attention launch is restated here from its launch site in kernels.hip, with att_mode's
default wave counts from policy.hip.  Every row must fit the 64 KB that a launch gets without
hipFuncAttributeMaxDynamicSharedMemorySize; every row marked `bound` must stop fitting four positions further; and
rau_create (device_id = -1: the configuration checks come before the device) must accept exactly what the
restatement accepts -- which holds att_max_pitch to the launches it stands for.  The labels of a row (trips of the q0
loop, lanes live in the last one, conv chunk depth and count, pad columns) are recomputed from its S.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from tests import range_cases as rc
from tests import test_gpu_bf16, util
from tests.test_gpu_positions import (ATT_ENV, B16, F32, LARGE, S_BF16_LARGE, S_MODULES_LARGE, SCALE, WAVE_ENV,
                                      large_id)

LDS_LAUNCH = 64 * 1024        # bytes, what a launch may request without the attribute
BATCH = {"split": 6, "split64": 64, "fused": 66, "fused6": 6}


# ---------------------------------------------------------------- the launches, restated
def family_split(B, env):                              # rau_ctx.hip att_family_split
    return "RAU_ATT_SPLIT" in env or (B <= 64 and "RAU_ATT_FUSED" not in env)


def waves(env, bf16, evaluate):                        # policy.hip att_mode
    one_of = lambda name: int(env[name]) if env.get(name) in ("8", "16") else 0
    return (one_of("RAU_ATT_WAVES_FWD") or (16 if evaluate else 8),
            one_of("RAU_ATT_WAVES_BWD") or (8 if bf16 else 16))


def lds_requests(B, A, pitch, bf16=False, env=None):
    """{launch: bytes of dynamic LDS} over a training step and an evaluate-mode step; pitch above 256, where the
    fused family runs its register-staged kernels (att_fwd_dma_ok / att_bwd_dma_ok: S <= 256)."""
    env = env or {}
    assert pitch % 4 == 0 and pitch > 256
    S = pitch
    if family_split(B, env):
        floats = {"k_att_score_part": 4 * S,           # att_fwd_split
                  "k_att_ctx": S + 8,
                  "k_att_da_part": 4 * S,              # att_bwd_split
                  "k_att_ds": S + 4}
    else:
        floats = {}
        for evaluate in (False, True):
            nf, nb = waves(env, bf16, evaluate)
            floats[f"k_att_fwd_fused<{nf}>"] = (nf + 2) * S + 2 * nf + A     # att_fwd_fused
            floats[f"k_att_bwd_fused<{nb}>"] = (nb + 1) * S + nb             # att_bwd_fused
    return {k: 4 * v for k, v in floats.items()}


def fits(B, A, pitch, bf16=False, env=None):
    return max(lds_requests(B, A, pitch, bf16, env).values()) <= LDS_LAUNCH


def largest_pitch(B, A, bf16=False, env=None):
    ok = [p for p in range(260, 8192, 4) if fits(B, A, p, bf16, env)]
    assert ok == list(range(260, ok[-1] + 4, 4))       # monotone: one bound
    return ok[-1]


def configurations():
    """[(id, B, A, bf16, env, S, bound)]: every context that section 7 of tests/test_gpu_positions.py creates."""
    out = [(f"{r.sec}-{large_id(r)}", BATCH[r.sec], r.over.get("A", F32["A"]), False, r.env, r.S, r.bound)
           for r in LARGE]
    out += [(f"bf16-{S}-{mode}", B16["B"], B16["A"], True, {}, S, S == 4096) for S, mode in S_BF16_LARGE]
    out += [(f"modules-{S}", 6, F32["A"], False, {}, S, S == 4096) for S in S_MODULES_LARGE]
    return out


CONFIGS = configurations()


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_a_row_fits_and_a_bound_row_is_the_last_that_does(cfg):
    _, B, A, bf16, env, S, bound = cfg
    pitch = (S + 3) & ~3
    req = lds_requests(B, A, pitch, bf16, env)
    assert max(req.values()) <= LDS_LAUNCH, req
    over = {k: v for k, v in lds_requests(B, A, pitch + 4, bf16, env).items() if v > LDS_LAUNCH}
    assert bool(over) == bound, (req, over)
    if bound:
        assert pitch == largest_pitch(B, A, bf16, env)


def test_the_bounds_and_what_binds_at_them():
    """The figures of the README and DESIGN.md section 3, from the restatement."""
    assert largest_pitch(6, 128) == largest_pitch(64, 16) == 4096
    assert lds_requests(6, 128, 4096)["k_att_score_part"] == LDS_LAUNCH
    assert [largest_pitch(66, A) for A in (128, 256, 16)] == [900, 892, 904]
    assert largest_pitch(66, 128, env={"RAU_ATT_WAVES_FWD": "8"}) == 960
    assert largest_pitch(66, 64, bf16=True) == 904 and largest_pitch(6, 128, env={"RAU_ATT_FUSED": "1"}) == 900
    binds = lambda req: max(req, key=req.get)
    assert binds(lds_requests(66, 128, 900)) == "k_att_fwd_fused<16>"          # the evaluate-mode forward
    assert binds(lds_requests(66, 128, 960, env={"RAU_ATT_WAVES_FWD": "8"})) == "k_att_bwd_fused<16>"
    # train mode alone would launch up to the backward's 960: only a context that never evaluates could use them
    assert lds_requests(66, 128, 904)["k_att_fwd_fused<8>"] <= LDS_LAUNCH < lds_requests(66, 128, 904)["k_att_fwd_fused<16>"]


KEYS = sorted({(B, A, bf16, tuple(sorted(env.items()))) for _, B, A, bf16, env, _, _ in CONFIGS})


@pytest.mark.parametrize("B,A,bf16,env", KEYS, ids=[f"B{B}-A{A}{'-bf16' if h else ''}{''.join('-' + k for k, _ in e)}"
                                                    for B, A, h, e in KEYS])
def test_create_accepts_exactly_what_the_launches_can_request(monkeypatch, B, A, bf16, env):
    from rau_vqa_amd import _lib
    for k in ATT_ENV + WAVE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    lib = _lib.lib()
    top = largest_pitch(B, A, bf16, dict(env))

    def refused(S):
        cfg = _lib.RauConfig()
        lib.rau_default_config(C.byref(cfg))
        for k, v in dict(F32, B=B, A=A, S=S, dtype=int(bf16), device_id=-1).items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        ret = lib.rau_create(C.byref(cfg), C.byref(h))
        msg = lib.rau_last_error()
        assert not h.value
        if b"64 KB" in msg:
            assert ret == -1 and b"above the %d positions" % top in msg, msg      # RAU_ERR_INVALID
            return True
        # past the configuration checks: stopped at the device (none here: RAU_ERR_DEVICE) or at its id
        assert (ret == -2 and b"no HIP device" in msg) or (ret == -1 and b"device_id" in msg), (ret, msg)
        return False
    assert [refused(S) for S in (top - 3, top, top + 1, top + 4)] == [False, False, True, True]


# ---------------------------------------------------------------- the labels
@pytest.mark.parametrize("row", LARGE, ids=[f"{r.sec}-{large_id(r)}" for r in LARGE])
def test_a_row_states_what_its_S_gives(row):
    pitch = (row.S + 3) & ~3
    s4 = pitch // 4
    trips = -(-s4 // 64)                               # for (q0 = 0; q0 < S4; q0 += 64)
    depth = 28 if pitch % 28 == 0 else 32              # gemm_conv.hip conv_wgrad_any, f32
    assert (row.pitch, row.trips, row.lanes, row.depth, row.chunks, row.pad) == \
        (pitch, trips, s4 - 64 * (trips - 1), depth, -(-pitch // depth), pitch - row.S)
    assert row.S > 400 and row.why and set(row.over) <= {"D", "M", "A"} and all(v % 4 == 0 for v in row.over.values())


def test_the_table_covers_what_it_claims():
    assert len({(r.sec, large_id(r)) for r in LARGE}) == len(LARGE)
    assert {r.sec for r in LARGE} == set(BATCH)
    for sec in ("split", "fused"):
        rows = [r for r in LARGE if r.sec == sec]
        assert {r.trips for r in rows} >= {2, 3, 4}, sec
        assert any(r.lanes == 64 for r in rows) and any(r.lanes == 1 for r in rows), sec    # a trip that ends exactly
        assert {r.depth for r in rows} == {28, 32} and any(r.pad == 3 and r.bound for r in rows), sec
        assert any(r.bound and r.pad == 0 and not r.over and not r.env for r in rows), sec
    split = [r for r in LARGE if r.sec == "split"]
    assert {8, 16} <= {r.trips for r in split} and max(r.chunks for r in split) == 146
    assert any(0 < r.lanes < 64 and r.trips == 16 for r in split)
    fused = [r for r in LARGE if r.sec == "fused"]
    assert {r.over.get("A", 128) for r in fused if r.bound} == {16, 128, 256}
    assert any(r.bound and "RAU_ATT_WAVES_FWD" in r.env for r in fused)


# ---------------------------------------------------------------- bf16 mode: what the emulation alone reaches
@pytest.mark.parametrize("S,mode", S_BF16_LARGE)
def test_bf16_rows_are_reachable_by_the_emulation(S, mode):
    """tests/test_gpu_bf16.run's two bars with the f32 run of the rounding emulation in the device's place
    (tests/test_range_host.py does the same for the value-range scenarios): a row that the emulation cannot hold
    inside them would say nothing about the device."""
    tb = test_gpu_bf16
    sh = util.shapes(dict(B16, S=S))
    b, params, masks = util.make_problem(sh, scale=SCALE)
    args = (sh, params, b["feats"], b["tokens"], b["lens"], b["labels"], masks if mode == "train" else None,
            rc.hop_weights(sh))
    exact = RT.step(*args, per_sample_abs=True)
    emu = RT.step(*args, bf16=True)
    stand_in = RT.step(*args, bf16=True, dtype=torch.float32)
    flips = [rc.errors(RT.step(*args, bf16=True, bf16_nudge=n), emu, sh) for n in tb.NUDGES]
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    e = rc.errors(stand_in, emu, sh)
    r1 = max(e[k] / (tb.TOL_BASE + one_flip + tb.SAFETY * max(f[k] for f in flips)) for k in e)
    r2 = 0.0
    for key, grp, sl in rc.slices(sh):
        if grp is None:
            r2 = max(r2, rc.slice_err(stand_in[key], exact[key]) / tb.TOL_EXACT)
        else:
            g, r = stand_in[grp][sl], exact[grp][sl]
            scale = max(float(np.max(np.abs(r))), float(np.max(exact["gabs_" + grp[2:]][sl])))
            d = float(np.max(np.abs(g - r)))
            r2 = max(r2, (d / scale if scale > 1e-12 else d) / tb.TOL_EXACT_GRAD)
    print(f"S={S} {mode}: emulation in f32 / derived bar {r1:.3f}, / exact-oracle bar {r2:.3f}")
    assert r1 < 1 and r2 < 1, (r1, r2)
