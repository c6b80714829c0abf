"""The value-range scenarios of tests/range_cases.py, without a device: each one reaches its regime, the two fp64
oracles agree on it, and the two f32 restatements stay finite and within TOL / 2 = 5e-5 of fp64 on every slice of
every single-site scenario -- the condition that keeps the device bar max(TOL, 4 e32) of tests/test_gpu_range.py from
loosening past 2e-4.  A scenario that breaks it is weakened (range_cases.TOP_EVERY is such a weakening), never the bar.

Measured (F32 dims, B = 6, largest slice error of the two f32 restatements, train / evaluate mode):
  peak_first 5.8e-7 / 5.9e-7    peak_last 5.6e-7 / 4.5e-7       peak_before_pad 7.0e-7 / 5.0e-7
  peak_before_count 6.4e-7 / 5.6e-7   peak_second_trip 7.1e-7 / 9.8e-7   two_peaks 1.7e-6 / 6.6e-7
  sat_i_embed 2.8e-6 / 2.2e-6   sat_addfeat 2.9e-6 / 2.2e-6     sat_att_lstm 1.9e-6 / 5.2e-6
  sat_encoder 5.3e-6 / 2.3e-6   sat_q_embed 2.9e-6 / 5.2e-6     big_logits_top 1.0e-5 / 3.4e-6
  big_logits_bottom 3.7e-5 / 2.3e-5 (att_score.b)               combined (not capped) 8.2e-6 / 9.6e-6
  above 400 positions: peak_last_4096 7.1e-7 / 4.6e-7   peak_before_pad_4093 6.1e-7 / 5.1e-7   two_peaks_4096 2.8e-6 /
  2.8e-6 (att_mem.b)   peak_third_trip_772 6.8e-7 / 7.4e-7   peak_last_900 4.4e-7 / 5.1e-7   peak_before_pad_897
  5.3e-7 / 5.5e-7   peak_before_count_900 9.8e-7 / 6.8e-7
The two fp64 oracles: at most 2.5e-13 absolute (combined, logits of magnitude 338).
"""
import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from tests import range_cases as rc
from tests import test_gpu_bf16, util

TOL_AGREE = 1e-10      # tests/test_oracle_agree.py's bar
HALF_TOL = 5e-5        # tests/test_gpu_parity.TOL / 2

MODES = ("train", "eval")
SINGLE = [n for n, s in rc.SCENARIOS.items() if s.single_site]


def test_the_layout_is_the_oracles_own():
    """views() walks ref_torch's specs and must cover the flat groups exactly; writing through a view lands in params."""
    p = rc.problem("peak_first")
    v = rc.views(p.sh, p.params)
    assert v["att_mem.b"].base is not None and v["att_mem.b"].shape == (p.sh.S,)
    assert v["att_mem.b"][0] == rc.PEAK_C and np.all(v["att_mem.b"][1:] == -rc.PEAK_C)
    assert {k for k, g, _ in rc.slices(p.sh) if g} == set(v)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(rc.SCENARIOS))
def test_regime(name, mode):
    p = rc.problem(name, mode)
    res = rc.SCENARIOS[name].regime(p, rc.reference(name, mode))
    print(f"{name} {mode}:", "; ".join(res))
    assert res and all(res.values()), [k for k, ok in res.items() if not ok]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(rc.SCENARIOS))
def test_the_two_fp64_oracles_agree(name, mode):
    """The hand-derived C++ backward against autograd at these values, tests/test_oracle_agree.py's way."""
    a, b = rc.reference(name, mode, which="cpp64"), rc.reference(name, mode)
    for k in util.OUT_KEYS + util.GRAD_KEYS:
        assert np.all(np.isfinite(b[k])), k
        err = float(np.max(np.abs(np.asarray(a[k], np.float64) - b[k])))
        assert err < TOL_AGREE, (k, err)
    assert np.array_equal(a["argmax"], b["argmax"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SINGLE)
def test_f32_restatements_within_half_the_bar(name, mode):
    ref = rc.reference(name, mode)
    for which in ("t32", "c32"):
        r = rc.reference(name, mode, which=which)
        assert r is not ref and r["logits"].dtype == np.float32 and r["g_mult"].dtype == np.float32, which
        for k in util.OUT_KEYS + util.GRAD_KEYS:
            assert np.all(np.isfinite(r[k])), (which, k)
    e = rc.e32(name, mode)
    assert min(e["logits"], e["att_c"]) > 0, "an f32 restatement without an f32 error is not one"
    worst = max(e, key=e.get)
    print(f"{name} {mode}: largest f32 error {e[worst]:.2e} ({worst})")
    assert e[worst] <= HALF_TOL, {k: v for k, v in e.items() if v > HALF_TOL}


@pytest.mark.parametrize("mode", MODES)
def test_combined_scenario_is_recorded_not_capped(mode):
    for which in ("t32", "c32"):
        r = rc.reference("combined", mode, which=which)
        assert all(np.all(np.isfinite(r[k])) for k in util.OUT_KEYS + util.GRAD_KEYS), which
    e = rc.e32("combined", mode)
    worst = max(e, key=e.get)
    print(f"combined {mode}: largest f32 error {e[worst]:.2e} ({worst})")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", rc.BF16_CASES)
def test_bf16_rows_are_reachable_by_the_emulation(name, mode):
    """tests/test_gpu_bf16.run's two bars with the f32 run of the rounding emulation in the device's place: a scenario
    that the emulation itself cannot hold inside them says nothing about the device.  The regime must hold at the
    bf16 dims too."""
    tb = test_gpu_bf16
    p = rc.problem(name, mode, dims=rc.B16)
    sh, b = p.sh, p.batch
    args = (sh, p.ref_params(), b["feats"], b["tokens"], b["lens"], b["labels"],
            p.masks if mode == "train" else None, rc.hop_weights(sh))
    exact = RT.step(*args, per_sample_abs=True)
    res = rc.SCENARIOS[name].regime(p, exact)
    assert all(res.values()), res
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
    print(f"{name} {mode}: emulation in f32 / derived bar {r1:.3f}, / exact-oracle bar {r2:.3f}")
    assert r1 < 1 and r2 < 1, (r1, r2)
