"""Parity over the value range: peaked attention, saturated gates, big logits (tests/range_cases.py has the scenarios
and their regime predicates, tests/test_range_host.py what the references alone do on them).

1. The step path against fp64 on every scenario, through tests/test_gpu_parity.check with the prepared problem: its
   1e-4 bar holds on every slice, which is at or below the bar this file states, max(TOL, 4 e32) per slice -- e32 the
   larger of the two f32 restatements' errors on that slice, from the references alone (at most 2e-4 on a single-site
   scenario, tests/test_range_host.py).  `error / bar` is printed per case.  Beyond the max-norm: everything finite,
   attention >= 0 with rows summing to 1 within 1e-6, pad columns and positions behind a region count exactly +0, a
   placed peak exactly 1.0f (two: 0.5f / 0.5f) and exactly 0 elsewhere, the attention argmax fp64's.  The peaks above
   400 positions (range_cases.PEAKS_ABOVE_400) run in the split family to 4096 and in the fused one to its bound of 900.
2. bf16 mode through tests/test_gpu_bf16.run, bars unchanged; the rows are range_cases.BF16_CASES.
3. The consumers of big logits: loss rows, rau_step_stats' merged losses, rau_topk's confidences, the answer-set
   criterion, rau_backward_merged.
4. The primitives alone, read out through module-level calls: tanh_fast and 1 - t^2 (embedding), sigmoidf_ (DeepLSTM
   cell, forward and backward), k_ce_fwd and the answer-set criterion on caller-supplied logits, rau_dev_rowmax on a
   row without an element above -inf.
"""
import ctypes as C

import numpy as np
import pytest

from tests import range_cases as rc
from tests import test_gpu_bf16, test_gpu_parity, util
from tests.test_gpu_parity import TOL
from tests.test_gpu_positions import ATT_ENV

pytestmark = pytest.mark.gpu

MODES = ("train", "eval")
FUSED_ENVS = {"FUSED": {"RAU_ATT_FUSED": "1"}, "FUSED DMA_OFF": {"RAU_ATT_FUSED": "1", "RAU_ATT_DMA_OFF": "1"}}
# the fused family and its register-staged form at B = 6: every placed peak, saturated addfeat, combined
FUSED_CASES = tuple(n for n in rc.PEAKS if n not in rc.PEAKS_ABOVE_400) + ("sat_addfeat", "combined")
# the peaks above 400 positions that the fused family can be created for (the others are the split family's alone);
# RAU_ATT_DMA_OFF changes nothing above 256 positions
FUSED_ABOVE_400 = tuple(n for n in rc.PEAKS_ABOVE_400 if rc.SCENARIOS[n].S <= rc.FUSED_MAX_S)
STEP_CASES = tuple(n for n in rc.SCENARIOS if n not in ("sat_i_embed_bf16", "sat_i_embed_tied"))


# ---------------------------------------------------------------- 1. the step path
def pitched(m, t):
    """The [H, n, Sp] buffer behind output_tensors()' attention view, downloaded."""
    import torch
    H, n, Sp = m.cfg.H, m.batch_size, (m.cfg.S + 3) & ~3
    m.sync()
    return torch.as_strided(t, (H, n, Sp), (n * Sp, Sp, 1)).cpu().numpy()


def step_case(monkeypatch, name, mode, B=6, env=None, tied=False):
    """tests/test_gpu_parity.check on the scenario's prepared problem against the shared fp64 reference, then the
    properties a max-norm does not see.  Returns the device's outputs."""
    from oracle import ref_torch
    from rau_vqa_amd import model
    for k in ATT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    p = rc.problem(name, mode, B)
    ref = rc.reference(name, mode, B)
    for which in ("t32", "c32"):        # both f32 restatements, before anything stands in for ref_torch.step
        assert rc.reference(name, mode, B, which)["logits"].dtype == np.float32
    seen = {}

    class Ranged(model.RAU):
        """The scenario's region counts on every batch; with `tied`, one x mask for all hops."""

        def training(self):
            super().training()
            if tied:
                self.tie_feature_dropout()

        def set_masks(self, masks):
            super().set_masks(dict(masks, x=np.ascontiguousarray(masks["x"][0])) if tied else masks)

        def set_batch(self, *a, **kw):
            super().set_batch(*a, regions=p.regions, **kw)

        def outputs(self):
            out = super().outputs()
            out["att_pitched"] = pitched(self, self.output_tensors()[2])
            return out

    real_run = test_gpu_parity.run_gpu

    def run_gpu(*a, **kw):
        out, layouts = real_run(*a, **kw)
        seen.update(out=out, layouts=layouts)
        return out, layouts
    monkeypatch.setattr(model, "RAU", Ranged)
    monkeypatch.setattr(test_gpu_parity, "run_gpu", run_gpu)
    monkeypatch.setattr(ref_torch, "step", lambda *a, **kw: ref)      # computed once, shared by the families
    try:
        errs = test_gpu_parity.check(p.sh, mode=mode, torch_oracle=True, problem=(p.batch, p.params, p.masks))
    finally:
        if "out" in seen:
            report(name, mode, B, env, p, ref, seen)
    got = seen["out"]
    assert set(errs) == set(rc.errors(got, ref, p.sh, seen["layouts"]))
    properties(p, ref, got)
    return got


def report(name, mode, B, env, p, ref, seen):
    errs = rc.errors(seen["out"], ref, p.sh, seen["layouts"])
    e32 = rc.e32(name, mode, B, seen["layouts"])
    ratio = {k: errs[k] / max(TOL, 4 * e32[k]) for k in errs}
    worst = max(ratio, key=ratio.get)
    fam = " ".join(sorted(env or {})) or "default"
    print(f"{name} B={B} {mode} [{fam}]: largest error / bar {ratio[worst]:.3f} ({worst}: {errs[worst]:.2e}, "
          f"e32 {e32[worst]:.2e})")


def properties(p, ref, got):
    sh = p.sh
    for k in util.OUT_KEYS + util.GRAD_KEYS:
        assert np.all(np.isfinite(got[k])), k
    att = got["att"]
    assert att.dtype == np.float32 and np.all(att >= 0)
    assert np.max(np.abs(att.sum(axis=2, dtype=np.float64) - 1)) <= 1e-6
    plus_zero = lambda a: not a.size or (np.all(a == 0) and not np.any(np.signbit(a)))
    assert plus_zero(got["att_pitched"][:, :, sh.S:]), "pad columns"
    assert np.array_equal(got["att_pitched"][:, :, :sh.S], att)
    if p.regions is not None:
        for b, n in enumerate(p.regions):
            assert plus_zero(att[:, b, n:]), "behind the region count"
    if p.peaks:
        share = np.float32(1.0 / len(p.peaks))
        for s in p.peaks:
            assert np.all(att[:, :, s] == share), (s, att[:, :, s])
        assert plus_zero(np.delete(att, p.peaks, axis=2)), "beside the peaks"
    # the attention argmax is fp64's on EVERY row: fp64 decides every row of every committed case (top-2 gap above
    # 1e-5 of the top, util.argmax_margin_ok's margin of 25 x the f32 error -- asserted, so a case that stops deciding
    # a row fails here instead of going unchecked); two equal peaks are a tie that the first position wins in both
    srt = np.sort(ref["att"], axis=2)
    decided = srt[..., -1] - srt[..., -2] > 1e-5 * srt[..., -1]
    assert decided.all() or len(p.peaks) == 2, f"fp64 leaves {(~decided).sum()} attention rows undecided"
    if len(p.peaks) != 2:
        assert np.array_equal(att.argmax(axis=2), ref["att"].argmax(axis=2))
    else:
        assert np.all(att.argmax(axis=2) == min(p.peaks)) and np.all(ref["att"].argmax(axis=2) == min(p.peaks))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", STEP_CASES)
def test_split_family(monkeypatch, name, mode):
    """B = 6: the split attention family, every scenario."""
    step_case(monkeypatch, name, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env", sorted(FUSED_ENVS))
@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_family(monkeypatch, name, env, mode):
    """The LDS-DMA kernels up to 256 positions, the register-staged ones above them or with RAU_ATT_DMA_OFF."""
    step_case(monkeypatch, name, mode, env=FUSED_ENVS[env])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FUSED_ABOVE_400)
def test_fused_family_above_400_positions(monkeypatch, name, mode):
    """The register-staged pair at B = 6, up to the family's bound of 900 positions."""
    step_case(monkeypatch, name, mode, env=FUSED_ENVS["FUSED"])


@pytest.mark.parametrize("name", ["combined", "peak_first"] + list(FUSED_ABOVE_400))
def test_large_batch(monkeypatch, name):
    """B = 66: the fused family and the `light` policies without a knob."""
    step_case(monkeypatch, name, "train", B=66)


def test_tied_feature_dropout(monkeypatch):
    """I and the attention pre-activation computed once, tied_bwd.hip summing the hops, on a saturated I."""
    step_case(monkeypatch, "sat_i_embed_tied", "train", tied=True)


def test_captured_step_is_the_eager_step(monkeypatch):
    """graph_step on the combined scenario: bit-equal to zero_grads + forward + backward."""
    from rau_vqa_amd.model import RAU, Config
    for k in ATT_ENV:
        monkeypatch.delenv(k, raising=False)
    p = rc.problem("combined", "train")
    sh, b = p.sh, p.batch
    res = []
    for graph in (False, True):
        m = RAU(Config(**{k: getattr(sh, k) for k in
                          ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H",
                           "p_we", "p_rnn", "p_q", "p_x", "p_mf")}))
        m.set_params(p.params)
        m.training()
        m.set_masks(p.masks)
        m.set_batch(b["feats"], b["tokens"], b["lens"], b["labels"])
        if graph:
            m.graph_step(rc.hop_weights(sh))
        else:
            m.zero_grads()
            m.forward()
            m.backward(rc.hop_weights(sh))
        out = m.outputs()
        g = m.get_grads()
        out.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]})
        res.append(out)
        m.close()
    for k in util.OUT_KEYS + ("argmax",) + util.GRAD_KEYS:
        assert np.all(np.isfinite(res[0][k])), k
        assert np.array_equal(res[0][k], res[1][k]), k


# ---------------------------------------------------------------- 2. bf16 mode
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", rc.BF16_CASES)
def test_bf16(name, mode):
    p = rc.problem(name, mode, dims=rc.B16)
    assert p.regions is None
    dims = {k: getattr(p.sh, k) for k in ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")}
    test_gpu_bf16.run(dims, rc.SCALE, mode, problem=(p.batch, p.params, p.masks))


# ---------------------------------------------------------------- 3. the consumers of big logits
def _bar(err32):
    return max(TOL, 4 * err32)


def _stats_losses(logits, dopred_gate, labels):
    """[H + 2]: the mean cross-entropy of every hop, of the uni row and of the select row (feval's rule: the first
    hop whose do_pred > 0.5, the zero row where none fires), in the dtype of logits; gates from dopred_gate."""
    from rau_vqa_amd import joint
    uni, select, _ = joint.merged_rows(logits, dopred_gate)
    rows = np.concatenate([logits, uni[None], select[None]])
    return rc.loss_rows(rows, labels).mean(axis=-1)


@pytest.fixture(scope="module", params=["big_logits_top", "big_logits_bottom"])
def big(request):
    """One train-mode forward on the big-logits problem; the context stays open for the tests that read it."""
    from tests.test_gpu_modules import make_model
    name = request.param
    p = rc.problem(name, "train")
    m = make_model(p.sh, p.params, p.masks)
    b = p.batch
    m.set_batch(b["feats"], b["tokens"], b["lens"], b["labels"])
    m.zero_grads()
    m.forward()
    yield name, p, m
    m.close()


def test_loss_rows_on_big_logits(big):
    name, p, m = big
    labels = p.batch["labels"]
    want = rc.loss_rows(rc.reference(name, "train")["logits"], labels)
    e32 = max(util.rel_err(rc.loss_rows(rc.reference(name, "train", which=w)["logits"], labels), want)
              for w in ("t32", "c32"))
    got = m.loss_rows()
    err = util.rel_err(got, want)
    print(f"{name}: loss rows error / bar {err / _bar(e32):.3f} (largest row {want.max():.1f}, smallest {want.min():.2e})")
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    assert err <= _bar(e32)


def test_step_stats_losses_on_big_logits(big):
    name, p, m = big
    ref = rc.reference(name, "train")
    labels = p.batch["labels"]
    assert np.array_equal(m.dopred() > 0.5, ref["dopred"] > 0.5), "a do_pred crossed 0.5: choose another seed"
    want = _stats_losses(ref["logits"], ref["dopred"], labels)
    e32 = max(util.rel_err(_stats_losses(rc.reference(name, "train", which=w)["logits"], ref["dopred"], labels), want)
              for w in ("t32", "c32"))
    got = m.step_stats()["loss"]
    err = util.rel_err(got, want)
    print(f"{name}: step_stats losses error / bar {err / _bar(e32):.3f} {want}")
    assert np.all(np.isfinite(got)) and err <= _bar(e32)


def test_topk_confidences_on_big_logits(big):
    """rau_topk against predict.top_answers (fp64 softmax of the device's own rows): tests/test_gpu_topk.conf_bound,
    per entry with the entry's own distance from the maximum, wherever the probability is above 1e-30."""
    from rau_vqa_amd import predict
    from tests.test_gpu_topk import U_EXP
    name, p, m = big
    K = p.sh.K
    tab_pred, _ = predict.merge_hops(m.logits(), m.dopred(), m.attention())
    rid, rscore, _ = predict.top_answers(tab_pred, K)
    ids, score, conf = m.topk(K)
    assert np.array_equal(ids, rid) and np.array_equal(score.view(np.uint32), rscore.view(np.uint32))
    x = rscore.astype(np.float64)
    soft = np.exp(x - x[..., :1]) / np.exp(x - x[..., :1]).sum(-1, keepdims=True)
    assert np.all(np.isfinite(conf)) and np.all(conf >= 0)
    bound = (2 * U_EXP + -(-K // 256) + 9 + 2 * (x[..., :1] - x)) * 2.0 ** -24
    live = soft >= 1e-30
    rel = np.abs(conf[live] - soft[live]) / soft[live]
    print(f"{name}: topk conf error / bound {np.max(rel / bound[live]):.3f}, spread {np.max(x[..., :1] - x):.0f}")
    assert np.all(rel <= bound[live]) and np.all(conf[~live] <= 1e-29)
    # the probabilities of a row sum to 1.  "At most 1" is out of reach of correctly rounded f32 values: rank 0 rounds
    # to 1.0f and the other ranks add positive amounts.  Each entry is within `bound` (relative) of its share, so the
    # sum exceeds 1 by at most sum_k soft_k bound_k -- below 1e-6 here, which is the bar; the largest sum is printed
    sums = conf.sum(-1, dtype=np.float64)
    print(f"{name}: largest topk row sum 1 + {sums.max() - 1:.2e}, allowed by the entries' bounds "
          f"{np.max((soft * bound).sum(-1)):.2e}")
    assert np.max((soft * bound).sum(-1)) <= 1e-6 and np.all(sums <= 1 + 1e-6)
    sure = x[..., 0] - x[..., 1] > 20
    assert sure.any() and np.all(np.abs(conf[..., 0][sure] - 1) <= 1e-6)


def _grad_check(name, got, ref, layouts, what):
    """Every layer slice within max(TOL, 4 e32); e32 is the scenario's own (the plain step's: the restatements with the
    extra term exist in fp64 only)."""
    e32 = rc.e32(name, "train", layouts=layouts)
    worst = 0.0
    for grp in ("embed", "rnn", "mult"):
        assert np.all(np.isfinite(got[grp])), grp
        for lname, sl in util.layer_slices(layouts[grp]):
            err = rc.slice_err(got[grp][sl], ref["g_" + grp][sl])
            worst = max(worst, err / _bar(e32[lname]))
            assert err <= _bar(e32[lname]), (what, lname, err, e32[lname])
    print(f"{name} {what}: largest gradient error / bar {worst:.3f}")


def test_merged_terms_on_big_logits(big):
    """rau_backward_merged with merge_w = [1, 1] against tests/merge_ref.py."""
    from tests import merge_ref
    name, p, m = big
    hop_w = rc.hop_weights(p.sh)
    ref = merge_ref.step(p.sh, p.params, p.batch, p.masks, hop_w, merge_w=[1.0, 1.0])
    m.zero_grads()
    m.forward()
    assert np.array_equal(merge_ref.first_fire(m.dopred()), ref["gate"]), "a do_pred crossed 0.5: choose another seed"
    m.backward(hop_w, merge_w=[1.0, 1.0])
    _grad_check(name, m.get_grads(), ref, {k: m.layout(k) for k in ("embed", "rnn", "mult")}, "merged")


def test_answer_set_on_big_logits(big):
    """G = 3 with one entry on the row's largest logit (of the last hop), the label and one more answer."""
    from tests import merge_ref
    name, p, m = big
    sh, b = p.sh, p.batch
    hop_w = rc.hop_weights(sh)
    logits64 = rc.reference(name, "train")["logits"]
    top = logits64[-1].argmax(axis=1) + 1
    ids = np.stack([top, b["labels"], (b["labels"] + 6) % sh.K + 1], axis=1).astype(np.int32)
    w = np.tile(np.array([0.5, 0.3, 0.2], np.float32), (sh.B, 1))
    ref = merge_ref.step(sh, p.params, b, p.masks, hop_w, answers=(ids, w))
    mx = logits64.max(axis=-1)
    lse = mx + np.log(np.exp(logits64 - mx[..., None]).sum(axis=-1))
    want = sum(float(w[0, g]) * (lse - np.take_along_axis(logits64, np.broadcast_to(ids[None, :, g:g + 1] - 1,
               logits64.shape[:2] + (1,)), axis=-1)[..., 0]) for g in range(3))
    try:
        m.set_batch(b["feats"], b["tokens"], b["lens"], b["labels"], answers=(ids, w))
        m.zero_grads()
        m.forward()
        rows = m.loss_rows()
        m.backward(hop_w)
        got = m.get_grads()
    finally:
        m.set_batch(b["feats"], b["tokens"], b["lens"], b["labels"])     # the fixture's batch, for the next test
        m.forward()
    e32 = rc.e32(name, "train")["logits"]
    err = util.rel_err(rows, want)
    print(f"{name}: answer-set loss rows error / bar {err / _bar(e32):.3f}")
    assert np.all(np.isfinite(rows)) and np.all(rows >= 0) and err <= _bar(e32)
    _grad_check(name, got, ref, {k: m.layout(k) for k in ("embed", "rnn", "mult")}, "answer set")


# ---------------------------------------------------------------- 4. the primitives alone
def _model(mode="eval", **dims):
    from tests.test_gpu_modules import make_model
    sh = util.shapes(dict(dict(B=2, T=1, V=4, E=4, Rq=4, D=4, S=4, M=4, A=4, R=4, K=4, H=1), **dims))
    _, params, _ = util.make_problem(sh, scale=0.1)
    return sh, params, make_model(sh, params, mode=mode)


def tanh_sweep():
    """The positive half of the sweep, ascending and distinct, float32."""
    eighth = np.float32(0.125).view(np.uint32)
    seam = (np.arange(-64, 65, dtype=np.int64) + int(eighth)).astype(np.uint32).view(np.float32)
    x = np.concatenate([
        np.array([0.0, 2.0 ** -149, 1e-30], np.float32),
        np.geomspace(1e-6, 0.125, 4096).astype(np.float32), seam,
        np.linspace(0.125, 12.0, 4096).astype(np.float32),
        np.array([20, 44, 45, 88, 89, 1e4, 1e30, np.finfo(np.float32).max], np.float32)])
    return np.unique(x)


@pytest.fixture(scope="module")
def tanh_readout():
    """tanh_fast and 1 - t^2 read out through rau_embed_forward / _backward: a V x E table of the sweep, one token
    per table row, evaluate mode (no mask), dwe = 1."""
    import torch
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda
    E = 16
    pos = tanh_sweep()
    x = np.concatenate([pos, -pos])
    V = -(-x.size // E)
    table = np.zeros(V * E, np.float32)
    table[:x.size] = x
    sh, params, m = _model(B=V, V=V, E=E)
    m.set_params(dict(params, embed=table))
    m.zero_grads()
    tok = cuda(np.arange(1, V + 1), torch.int32)
    clone = modules.EmbedClone(m, 0)
    t = clone.forward(tok)
    clone.backward(tok, cuda(np.ones((V, E), np.float32)))
    m.sync()
    t = t.cpu().numpy().reshape(-1)[:x.size]
    d = m.get_grads()["embed"][:x.size]
    m.close()
    n = pos.size
    return pos, t[:n], t[n:], d[:n], d[n:]


def test_tanh_fast(tanh_readout):
    """Measured: see LOG.md.  The budget of 2^-21 = 4.8e-7 (4 ulp of 1.0): the polynomial's truncation at 1/8
    (1.6e-10), a few roundings of values <= 1, the hardware exp's argument rounding (<= 5e-8 behind the
    2e / (e + 1)^2 attenuation), one division and one subtraction at magnitude <= 1."""
    x, tp, tn, _, _ = tanh_readout
    assert np.array_equal(tn.view(np.uint32), tp.view(np.uint32) ^ np.uint32(0x80000000)), "odd symmetry, bit for bit"
    assert x[0] == 0 and tp[0].view(np.uint32) == 0 and tn[0].view(np.uint32) == 0x80000000      # tanh(+-0) = +-0
    assert np.all(np.isfinite(tp)) and np.all(tp >= 0) and np.all(tp <= 1), "|t| <= 1: 1 - t^2 never negative"
    step = np.diff(tp.astype(np.float64))
    slack = np.where((x[1:] >= 0.125) & (x[1:] <= 12), 2.0 ** -24, 0.0)    # the division's rounding
    worst = int(np.argmin(step + slack))
    assert np.all(step + slack >= 0), (x[worst], x[worst + 1], tp[worst], tp[worst + 1])
    assert np.all(tp[x >= 10] == 1)
    err = np.abs(tp.astype(np.float64) - np.tanh(x.astype(np.float64)))
    k = int(np.argmax(err))
    seam = np.abs(x - 0.125) < 1e-6
    print(f"tanh_fast: largest |error| {err[k]:.3e} = {err[k] * 2 ** 24:.2f} x 2^-24 at x = {x[k]:.6g}; "
          f"below 1/8 {err[x < 0.125].max():.2e}, on the 129 floats around 1/8 {err[seam].max():.2e}, "
          f"largest backward step {-(step.min()):.2e}")
    assert err[k] <= 2.0 ** -21


def test_tanh_derivative_from_the_output(tanh_readout):
    """1 - t^2 as the backward passes form it from the stored output: 2 |t| dt with dt <= 2^-21 stays below 1e-6."""
    x, _, _, dp, dn = tanh_readout
    want = 1 - np.tanh(x.astype(np.float64)) ** 2
    for d in (dp, dn):
        assert np.all(np.isfinite(d)) and np.all(d >= 0)
        assert np.max(np.abs(d - want)) <= 1e-6
    assert np.array_equal(dp, dn)
    print(f"1 - t^2: largest |error| {np.max(np.abs(dp - want)):.3e}")


RQ = 512


def gate_sweep():
    """2 RQ biases in [-110, 110], ascending: where expf(-x) overflows or goes subnormal, where the result becomes 1."""
    special = np.array([16, 17, 18, 87, 88, 89, 104, 110], np.float32)
    special = np.concatenate([special, -special])
    # an even grid over the whole range: the midpoints of n equal cells (n even: no midpoint is an integer)
    n = 2 * RQ - special.size
    grid = (-110 + 220 * (np.arange(n) + 0.5) / n).astype(np.float32)
    x = np.unique(np.concatenate([special, grid]))
    assert x.size == 2 * RQ and x[0] == -110 and x[-1] == 110
    return x


def lstm_case(kind):
    """Zero weights; (rnn parameters, state [2, 4 RQ], sweep).  "in": in-transform bias +30 and previous c = 0, the
    in gate's bias sweeps: next_c is the sigmoid.  "forget": in gate at -110 (exactly 0), the forget gate's bias
    sweeps over a previous c of +1e3 (row 0) and -1e3 (row 1): next_c = sigmoid * c."""
    sh = util.shapes(dict(B=2, T=1, V=4, E=4, Rq=RQ, D=4, S=4, M=4, A=4, R=4, K=4, H=1))
    sweep = gate_sweep()
    params = {"rnn": np.zeros(sum(o * i + o for _, o, i in rc.ref_torch.rnn_specs(sh)), np.float32)}
    v = rc.views(sh, dict(params, mult=np.zeros(sum(o * i + o for _, o, i in rc.ref_torch.mult_specs(sh)), np.float32),
                          embed=np.zeros(sh.V * sh.E, np.float32)))
    state = np.zeros((2, 4 * RQ), np.float32)
    for layer, n in enumerate(("l1_i2h.b", "l2_i2h.b")):
        b4 = v[n].reshape(4, RQ)                       # in, forget, out, in-transform
        if kind == "in":
            b4[0], b4[3] = sweep[layer * RQ:(layer + 1) * RQ], 30.0
        else:
            b4[0], b4[1] = -110.0, sweep[layer * RQ:(layer + 1) * RQ]
            state[0, 2 * layer * RQ:(2 * layer + 1) * RQ] = 1e3
            state[1, 2 * layer * RQ:(2 * layer + 1) * RQ] = -1e3
    return sh, params["rnn"], state, sweep


@pytest.fixture(scope="module", params=["in", "forget"])
def lstm_readout(request):
    """rau_deeplstm_forward and _backward on lstm_case's inputs, with autograd on ref_torch.deep_lstm in fp64 and f32."""
    import torch
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda
    RT = rc.ref_torch
    kind = request.param
    sh, rnn, state, sweep = lstm_case(kind)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, sh.E)).astype(np.float32)
    gstate = rng.standard_normal((2, 4 * RQ)).astype(np.float32)
    _, params, m = _model(Rq=RQ)
    m.set_params(dict(params, rnn=rnn))
    m.zero_grads()
    clone = modules.DeepLSTMClone(m, 0)
    args = (cuda(x), cuda(state))
    out = clone.forward(*args)
    dx, ds = clone.backward(*args, cuda(gstate))
    m.sync()
    dev = dict(state=out.cpu().numpy(), d_x=dx.cpu().numpy(), d_state=ds.cpu().numpy(), g_rnn=m.get_grads()["rnn"])
    m.close()

    def autograd(dtype):
        t = lambda a: torch.as_tensor(a).to(dtype)
        flat = t(rnn).clone().requires_grad_(True)
        xi, st = t(x).requires_grad_(True), t(state).requires_grad_(True)
        o = RT.deep_lstm(sh, RT._split(flat, RT.rnn_specs(sh)), xi, st, None)
        o.backward(t(gstate))
        return dict(state=o.detach().numpy(), d_x=xi.grad.numpy(), d_state=st.grad.numpy(), g_rnn=flat.grad.numpy())
    return kind, sweep, state, dev, autograd(torch.float64), autograd(torch.float32)


def _next_c(out):
    """next_c of both layers side by side: [2, 2 RQ], in the sweep's order."""
    return np.concatenate([out[:, :RQ], out[:, 2 * RQ:3 * RQ]], axis=1)


def test_sigmoid_through_the_lstm_cell(lstm_readout):
    kind, x, state, dev, f64, _ = lstm_readout
    c = _next_c(dev["state"])
    assert np.all(np.isfinite(dev["state"]))
    want = 1 / (1 + np.exp(-x.astype(np.float64)))
    if kind == "in":
        for row in c:
            assert np.all(row >= 0) and np.all(row <= 1)
            assert np.all(np.diff(row) >= 0), "monotone"
            assert np.all(row[x >= 17] == 1)
            err = np.abs(row - want)
            k = int(np.argmax(err))
            assert err[k] <= 2.0 ** -22, (x[k], row[k], want[k])
        print(f"sigmoidf_: largest |error| {err[k]:.3e} = {err[k] * 2 ** 24:.2f} x 2^-24 at x = {x[k]:.6g}")
    else:
        # c carries through unclamped: sigmoid * (+-1e3) to 1e-6 relative; below f32's normal range (x < -87.3) the
        # gate has no relative precision left, there the error is held to the smallest normal float times |c|
        ref = _next_c(f64["state"])
        assert np.array_equal(np.sign(c[0]), np.sign(-c[1])) and np.array_equal(np.abs(c[0]), np.abs(c[1]))
        assert np.max(np.abs(c)) == 1e3
        err = np.abs(c - ref)
        assert np.all(err <= 1e-6 * np.abs(ref) + 1e3 * 2.0 ** -126)
        print(f"forget gate over c = +-1e3: largest relative error {np.max(err[:, x > -87] / np.abs(ref[:, x > -87])):.3e}")


def test_lstm_backward_on_saturated_gates(lstm_readout):
    """Within max(1e-6 absolute, 4 x the f32 autograd's own error) of fp64 autograd, per tensor."""
    kind, _, _, dev, f64, f32 = lstm_readout
    for k in ("state", "d_x", "d_state", "g_rnn"):
        assert np.all(np.isfinite(dev[k])), k
        own = float(np.max(np.abs(f32[k] - f64[k])))
        err = float(np.max(np.abs(dev[k] - f64[k])))
        print(f"lstm backward [{kind}] {k}: error {err:.2e}, f32 autograd's {own:.2e}, largest |value| {np.abs(f64[k]).max():.1f}")
        if k != "state":
            assert err <= max(1e-6, 4 * own), k


# criterion rows: tests/test_gpu_bce.py's EXTREME entries, a constant row at +1e4, one logit 200 above the rest with the
# label on it and off it, -1e4 everywhere except the label
def criterion_rows(K):
    from tests.test_gpu_bce import EXTREME
    rng = np.random.default_rng(K)
    x = rng.standard_normal((7, K)).astype(np.float32)
    n = EXTREME.size
    x[0, :n] = EXTREME
    x[1, -n:] = EXTREME
    x[2, :n] = EXTREME[::-1]
    x[3] = 1e4
    x[4, 5] += 200
    x[5, 5] += 200
    x[6] = -1e4
    x[6, K - 1] = 0
    y = np.array([n, K - n + 1, 4, 9, 6, 7, K], np.int32)     # on +1e4, on -1e4, on 0, any, on the peak, off it, the label
    return x, y


def _lse32(x):
    mx = x.max(axis=-1, keepdims=True)
    return (mx[..., 0] + np.log(np.exp(x - mx).sum(axis=-1, dtype=x.dtype))).astype(x.dtype)


@pytest.mark.parametrize("K", [48, 1000])
@pytest.mark.parametrize("kind", ["labels", "set"])
def test_criterion_on_extreme_logits(K, kind):
    """k_ce_fwd (labels) and the answer-set criterion (G = 3, weights 0.5 / 0.3 / 0.2: entry 0 is the label) on
    caller-supplied logits.  Loss rows one at a time (a batch of one: the mean is the row) against fp64 on the same f32
    logits, within 4 x the error of the f32 statement mx + log(sum(exp(x - mx))) with a floor of 2 ulp(max |x|);
    the gradient of the whole batch against fp64 softmax - onehot."""
    import torch
    from rau_vqa_amd import _lib, modules
    from tests.test_gpu_modules import cuda
    x, y = criterion_rows(K)
    B = x.shape[0]
    ids = np.stack([y, y % K + 1, (y + 10) % K + 1], axis=1).astype(np.int32)
    w = np.tile(np.array([0.5, 0.3, 0.2], np.float32), (B, 1))
    if kind == "labels":
        ids, w = ids[:, :1], np.ones((B, 1), np.float32)
    G = ids.shape[1]
    _, _, m = _model(B=B, K=K)
    p = lambda t: C.c_void_p(t.data_ptr())

    def forward(lg, yy, ii, ww):
        if kind == "labels":
            return modules.CriterionClone(m, 0).forward(lg, yy)
        loss = C.c_float()
        _lib.check(m._lib.rau_criterion_forward_set(m._h, 0, p(lg), G, p(ii), p(ww), C.byref(loss)))
        return loss.value

    x64 = x.astype(np.float64)
    pick = lambda a: np.take_along_axis(a, ids - 1, axis=1)
    mx = x64.max(axis=1, keepdims=True)
    lse64 = mx[:, 0] + np.log(np.exp(x64 - mx).sum(axis=1))
    want = (w * (lse64[:, None] - pick(x64))).sum(axis=1)
    stated = (w * (_lse32(x)[:, None] - pick(x))).sum(axis=1, dtype=np.float32)
    x_d, y_d, ids_d, w_d = cuda(x), cuda(y, torch.int32), cuda(ids, torch.int32), cuda(w)
    # the gradient first, on the whole batch
    if kind == "labels":
        dl = modules.CriterionClone(m, 0).backward(x_d, y_d)
    else:
        out = C.c_void_p()
        _lib.check(m._lib.rau_criterion_backward_set(m._h, 0, p(x_d), G, p(ids_d), p(w_d), 1.0, C.byref(out)))
        dl = modules.CriterionClone(m, 0)._view(out, B, K)
    mean = forward(x_d, y_d, ids_d, w_d)
    m.sync()
    dl = dl.cpu().numpy().astype(np.float64)
    soft = np.exp(x64 - lse64[:, None])
    onehot = np.zeros((B, K))
    for g in range(G):
        np.add.at(onehot, (np.arange(B), ids[:, g] - 1), w[:, g].astype(np.float64))
    assert np.all(np.isfinite(dl)) and np.isfinite(mean)
    # [-1/B, 1/B] in the f32 factors the kernels form: invB = 1.f / B, W = the weights added in g order, p (W invB)
    # rounded once -- no entry can leave [-W invB, W invB] (p <= 1, one matching entry per logit), and none may
    invB = np.float32(1) / np.float32(B)
    W32 = np.float32(0)
    for g in range(G):
        W32 = np.float32(W32 + w[0, g])
    assert np.all(np.abs(dl) <= float(np.float32(W32 * invB)))
    print(f"K={K} {kind}: largest |row sum| {np.abs(dl.sum(axis=1)).max() * B:.2e} / B, "
          f"gradient error {np.abs(dl - (soft - onehot) / B).max() * B:.2e} / B")
    assert np.all(np.abs(dl.sum(axis=1)) <= K * 2.0 ** -24 / B)
    assert np.max(np.abs(dl - (soft - onehot) / B)) <= 1e-6 / B
    # the loss, row by row
    m.set_batch_size(1)
    for r in range(B):
        got = forward(cuda(x[r:r + 1]), cuda(y[r:r + 1], torch.int32), cuda(ids[r:r + 1], torch.int32), cuda(w[r:r + 1]))
        bound = max(4 * abs(float(stated[r]) - want[r]), 2 * float(np.spacing(np.abs(x[r]).max())))
        print(f"K={K} {kind} row {r}: loss {got:.6g}, fp64 {want[r]:.6g}, error / bound {abs(got - want[r]) / bound:.3f}")
        assert np.isfinite(got) and got >= 0
        assert abs(got - want[r]) <= bound
        if stated[r] == 0:
            assert got == 0, "exactly 0 where f32 leaves nothing"
    m.close()


def test_rowmax_of_a_row_without_an_element_above_minus_inf():
    """torch.max returns index 1 on a row of -inf; rau_dev_topk ranks id 1 first on it.  (bi kept its sentinel
    0x7fffffff, and bi + 1 overflowed to a negative index.)"""
    from rau_vqa_amd.modules import DevTensor
    _, _, m = _model()
    x = np.full((3, 70), -np.inf, np.float32)
    x[1, 69] = -3.0                                     # a control row: its only finite entry, in the second trip
    t = DevTensor.zeros(m, 3, 70).copy(x)
    v, i = t.max(2)
    tv, ti = t.topk(2)
    m.sync()
    assert i.numpy("int32").reshape(-1).tolist() == [1, 70, 1]
    assert v.numpy().reshape(-1).tolist() == [-np.inf, -3.0, -np.inf]
    assert ti.numpy("int32")[:, 0].tolist() == [1, 70, 1]
    assert np.array_equal(tv.numpy()[:, 0], v.numpy().reshape(-1))
    m.close()
