"""The merged answers as training terms (rau_backward_merged, rau_graph_step_merged, rau_merge_criterion_backward,
merge_grad.hip): w_uni CE(uni row) + w_sel CE(select row) in the step's objective.

The oracle is tests/merge_ref.py (ref_torch's loop restated in fp64 autograd with the two terms added), the machinery
tests/test_gpu_select.py's: its committed problems under their explicit masks, make_model, grad_errs, check_argmax,
TOL = 1e-4 per layer slice.

The condition every parity test asserts: the device's gates do_pred > 0.5 equal the oracle's on every row and hop, and
(H > 1) the batch holds a row that first fires at hop 0, one that first fires at a later hop and one that never fires.
Checked on the CPU for the committed problems (train mode, explicit masks):
  SMALL   {never: 3, hop 0: 2, hop 1: 3}       min |do_pred - 0.5| = 0.026
  MEDIUM  {never: 27, hop 0: 28, hop 1: 15}    min |do_pred - 0.5| = 1.6e-4
  EDGE    fires on all 5 rows (H = 1)          min |do_pred - 0.5| = 0.071
In evaluate mode no row fires at these seeds, so the select term is not tested there: it would be vacuous.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from tests import merge_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_select import (GROUPS, INVALID, STATE, TOL, check_argmax, f32, grad_errs, make_model, problem,
                                   same_bits, small_answer_set, targets)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ machinery
def ptr(a):
    return None if a is None else a.ctypes.data


def call(m, name, *args):
    from rau_vqa_amd._lib import check
    check(getattr(m._lib, name)(m._h, *args))


def step(m, hop_w, merge_w, select_w=None, att_w=None, how="merged"):
    """zero_grads + forward + backward through the named entry point (None is passed as NULL); the gradients."""
    hw = f32(hop_w)
    sw, aw, mw = (None if a is None else f32(a) for a in (select_w, att_w, merge_w))
    if how == "graph":
        call(m, "rau_graph_step_merged", ptr(hw), ptr(sw), ptr(aw), ptr(mw), 1)
    else:
        m.zero_grads()
        m.forward()
        if how == "merged":
            call(m, "rau_backward_merged", ptr(hw), ptr(sw), ptr(aw), ptr(mw))
        elif how == "att":
            call(m, "rau_backward_att", ptr(hw), ptr(sw), ptr(aw))
        else:
            call(m, "rau_backward", ptr(hw))
    return m.get_grads()


_FWD = {}


def oracle_forward(dims_name, answers=None):
    """The fp64 oracle's forward of the committed problem (logits, argmax, do_pred, gate): computed once, shared."""
    key = (dims_name, answers is not None)
    if key not in _FWD:
        sh, batch, params, masks = problem(dims_name)
        _FWD[key] = merge_ref.step(sh, params, batch, masks, [0.0] * sh.H, backward=False)
    return _FWD[key]


def check_gates(m, ref_fwd, H):
    """The condition: the device's gates equal the oracle's everywhere, and every kind of row occurs (H > 1)."""
    gate = merge_ref.first_fire(m.dopred())
    assert np.array_equal(m.dopred() > 0.5, ref_fwd["dopred"] > 0.5), "a do_pred crossed 0.5: choose another seed"
    assert np.array_equal(gate, ref_fwd["gate"])
    hist = merge_ref.fire_histogram(gate)
    if H > 1:
        assert hist["never"] > 0 and hist[0] > 0 and sum(hist[h] for h in range(1, H)) > 0, hist
    return hist


def put(m, batch, answers=None):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"],
                **({} if answers is None else {"answers": answers}))


def parity(dims_name, hop_w, merge_w, select_w=None, answers=None):
    sh, batch, params, masks = problem(dims_name)
    m = make_model(sh, params, masks)
    put(m, batch, answers)
    got = step(m, hop_w, merge_w, select_w)
    fwd = oracle_forward(dims_name)
    hist = check_gates(m, fwd, sh.H)
    t_gt = None
    if select_w is not None:
        t_gt = targets(check_argmax(m, fwd), batch, answers)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = merge_ref.step(sh, params, batch, masks, hop_w, merge_w, select_w, t_gt,
                         None if answers is None else answers[:2])
    errs = grad_errs(got, ref, layouts)
    print(hist, {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"
    return got, ref


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("dims_name,hop_w,merge_w,select_w", [
    ("SMALL", [3, 3, 3], [1, 0], None),
    ("SMALL", [3, 3, 3], [0, 1], None),
    ("SMALL", [3, 3, 3], [0.7, 1.3], None),
    ("SMALL", [0, 0, 0], [0.7, 1.3], None),               # the merged terms alone
    ("SMALL", [3, 3, 3], [0.7, 1.3], [0.7, 0, 1.3]),      # together with the selection head's BCE
    ("SMALL", [3, 0, 0], [0.7, 1.3], None),               # every hop is active whatever hop_w says
    ("EDGE", [1], [1, 0], None),
    ("EDGE", [1], [0, 1], None),
    ("EDGE", [1], [0.7, 1.3], None),
    ("MEDIUM", [2, 2], [0.7, 1.3], None),
])
def test_gradients_against_the_oracle(dims_name, hop_w, merge_w, select_w):
    parity(dims_name, hop_w, merge_w, select_w)


# ------------------------------------------------------------------------------------------ 2. answer set
def test_answer_set_both_terms():
    sh, batch, _params, _masks = problem("SMALL")
    parity("SMALL", [3, 3, 3], [0.7, 1.3], answers=small_answer_set(batch, sh))


# ------------------------------------------------------------------------------------------ 3. identity
def test_null_and_zero_merge_weights_are_rau_backward_att_bit_for_bit_and_launch_for_launch():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    put(m, batch)
    hop_w, sel_w = [3, 3, 3], [0.7, 0, 1.3]

    def run(*a, **k):
        m.prof_reset()
        g = step(m, *a, **k)
        m.sync()
        return g, {n: v["launches"] for n, v in m.prof().items() if v["launches"]}

    m.prof_enable()
    for sw in (None, sel_w):
        base, listing = run(hop_w, None, sw, None, how="att")
        assert "merge_grad" not in listing
        for mw in (None, [0, 0]):
            got, ls = run(hop_w, mw, sw, None, how="merged")
            same_bits(got, base)
            assert ls == listing
    plain, listing = run(hop_w, None, how="plain")
    got, ls = run(hop_w, None, None, None, how="merged")      # every optional argument NULL: rau_backward
    same_bits(got, plain)
    assert ls == listing
    got, ls = run(hop_w, [0.7, 1.3], None, None, how="merged")
    assert ls.get("merge_grad") == 1 and any(not np.array_equal(got[k], plain[k]) for k in GROUPS)
    m.prof_enable(False)
    same_bits(step(m, hop_w, None, how="graph"), plain)
    same_bits(step(m, hop_w, [0, 0], how="graph"), plain)
    # the Python forms
    m.zero_grads(); m.forward(); m.backward(f32(hop_w), merge_w=[0, 0])
    same_bits(m.get_grads(), plain)
    m.zero_grads(); m.forward(); m.backward(f32(hop_w), merge_w=[0.7, 1.3])
    same_bits(m.get_grads(), got)
    m.close()


# ------------------------------------------------------------------------------------------ 4. module level
def test_module_level_criterion_and_feval():
    from rau_vqa_amd import joint, modules
    sh, batch, params, masks = problem("SMALL")
    hop_w, merge_w = [3, 3, 3], [0.7, 1.3]
    m = make_model(sh, params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    put(m, batch)
    m.forward()
    lg, dp = m.logits(), m.dopred()
    hist = check_gates(m, oracle_forward("SMALL"), sh.H)
    cuda = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a)).cuda().to(dt or torch.float32)
    y = cuda(batch["labels"], torch.int32)
    d0 = np.random.default_rng(7).normal(size=lg.shape).astype(np.float32)
    never = merge_ref.first_fire(dp).sum(0) == 0
    d0[:, never, :4] = -0.0   # a negative zero keeps its sign where nothing is added
    with torch.cuda.stream(torch.cuda.ExternalStream(m.stream())):
        for mw in (merge_w, [1, 0], [0, 1.3]):
            for labels in (y, None):      # None: the resident batch's labels
                d = cuda(d0)
                modules.merge_criterion_backward(m, cuda(lg), cuda(dp), labels, mw, d)
                m.sync()
                got = d.cpu().numpy() - d0.astype(np.float64)
                want = joint.merged_ce_grad(lg, dp, labels=batch["labels"], merge_w=mw)
                assert util.rel_err(got, want) < TOL, mw
                if mw[0] == 0:   # rows on which no hop fired: the input's bits
                    assert hist["never"] > 0
                    assert np.array_equal(d.cpu().numpy()[:, never].view(np.uint32), d0[:, never].view(np.uint32))
        d = cuda(d0)
        modules.merge_criterion_backward(m, cuda(lg), cuda(dp), y, [0, 0], d)
        m.sync()
        assert np.array_equal(d.cpu().numpy().view(np.uint32), d0.view(np.uint32))
    # feval over the clones gives the step-level gradients
    m.zero_grads()
    _losses, answers = modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32),
                                     cuda(batch["lens"], torch.int32), y, f32(hop_w), merge_w=f32(merge_w))
    m.sync()
    g_mod = m.get_grads()
    assert np.array_equal(answers.cpu().numpy(), oracle_forward("SMALL")["argmax"])
    ref = merge_ref.step(sh, params, batch, masks, hop_w, merge_w)
    bad = {k: v for k, v in grad_errs(g_mod, ref, layouts).items() if not v < TOL}
    assert not bad, f"module-level feval above {TOL}: {bad}"
    m.close()


@pytest.mark.parametrize("K,H", [(4096, 2), (4100, 3)])
def test_both_sides_of_the_row_staging_threshold(K, H):
    """The two rows are kept in LDS up to K = 4096 (2 K floats = 32 KB) and recomputed above: the kernel on random
    hop outputs at both sides, labels and an answer set, against the numpy statement."""
    from rau_vqa_amd import joint, modules
    from rau_vqa_amd.model import RAU, Config
    B = 6
    m = RAU(Config(**dict(util.EDGE, B=B, K=K, H=H)))
    rng = np.random.default_rng(K)
    lg = rng.normal(size=(H, B, K)).astype(np.float32)
    dp = rng.uniform(size=(H, B)).astype(np.float32)
    dp[:, 0] = 0.2                                       # never fires
    dp[:, 1] = 0.9                                       # fires at hop 0
    dp[:, 2] = [0.1] * (H - 1) + [0.7]                   # first fires at the last hop
    y = rng.integers(1, K + 1, size=B).astype(np.int32)
    y[3], y[4] = 1, K                                    # the first and the last entry of a row
    ids = rng.integers(1, K + 1, size=(B, 3)).astype(np.int32)
    ids[:, 0] = y
    ids[5] = 0
    w = rng.uniform(0.1, 1.0, size=(B, 3)).astype(np.float32)
    d0 = rng.normal(size=lg.shape).astype(np.float32)
    cuda = lambda a: torch.as_tensor(a).cuda()
    with torch.cuda.stream(torch.cuda.ExternalStream(m.stream())):
        d = cuda(d0)
        modules.merge_criterion_backward(m, cuda(lg), cuda(dp), cuda(y), [0.7, 1.3], d)
        m.sync()
        got = d.cpu().numpy() - d0.astype(np.float64)
        assert util.rel_err(got, joint.merged_ce_grad(lg, dp, labels=y, merge_w=[0.7, 1.3])) < TOL
        # the answer set of the resident batch (labels_dev = NULL)
        feats = np.zeros((B, util.EDGE["D"], util.EDGE["S"]), np.float32)
        tokens = np.ones((util.EDGE["T"], B), np.int32)
        m.set_batch(feats, tokens, np.ones(B, np.int32), y, answers=(ids, w, w))
        d = cuda(d0)
        modules.merge_criterion_backward(m, cuda(lg), cuda(dp), None, [0.7, 1.3], d)
        m.sync()
        got = d.cpu().numpy() - d0.astype(np.float64)
        assert util.rel_err(got, joint.merged_ce_grad(lg, dp, answers=(ids, w), merge_w=[0.7, 1.3])) < TOL
        assert np.all(got[:, 5] == 0)                    # an unlabelled row
    m.close()


# ------------------------------------------------------------------------------------------ 5. graph step
def test_graph_step_replays_with_new_merge_weights():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    put(m, batch)
    hop_w = [3, 3, 3]
    for mw in ([0.7, 1.3], [0.2, 2.0]):                   # capture, then a replay at other values
        same_bits(step(m, hop_w, mw, how="graph"), step(m, hop_w, mw, how="merged"))
    same_bits(step(m, hop_w, None, how="graph"), step(m, hop_w, None, how="plain"))   # a NULL step in between
    same_bits(step(m, hop_w, [0.7, 1.3], how="graph"), step(m, hop_w, [0.7, 1.3], how="merged"))
    same_bits(step(m, hop_w, [0.7, 1.3], [0.7, 0, 1.3], how="graph"),
              step(m, hop_w, [0.7, 1.3], [0.7, 0, 1.3], how="merged"))
    m.zero_grads()
    m.graph_step(f32(hop_w), merge_w=[0.2, 2.0])          # the Python form
    same_bits(m.get_grads(), step(m, hop_w, [0.2, 2.0], how="merged"))
    m.close()


# ------------------------------------------------------------------------------------------ 6. bf16 mode
def test_bf16_mode_against_the_emulated_oracle():
    sh, batch, params, masks = problem("SMALL")
    hop_w, merge_w = [3, 3, 3], [0.7, 1.3]
    m = make_model(sh, params, masks, dtype="bf16")
    put(m, batch)
    got = step(m, hop_w, merge_w)
    layouts = {k: m.layout(k) for k in GROUPS}
    with RT.bf16_emulation():
        emu = merge_ref.step(sh, params, batch, masks, hop_w, merge_w, bf16=True)
    check_gates(m, emu, sh.H)
    m.close()
    nudged = []
    for n in NUDGES:
        with RT.bf16_emulation(n):
            nudged.append(merge_ref.step(sh, params, batch, masks, hop_w, merge_w, bf16=True))
    for x in nudged:   # the nudges move no gate either: the derived bar compares like with like
        assert np.array_equal(x["gate"], emu["gate"])
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    err = lambda a, b: float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    bad, ratio = {}, 0.0
    for grp in GROUPS:
        for name, sl in util.layer_slices(layouts[grp]):
            r = emu["g_" + grp][sl]
            flip = max(err(x["g_" + grp][sl], r) for x in nudged)
            tol = TOL_BASE + one_flip + SAFETY * flip
            e = err(got[grp][sl], r)
            ratio = max(ratio, e / tol)
            if not e < tol:
                bad[name] = (e, tol)
    print(f"bf16 merged: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated oracle, (error, derived bar): {bad}"


# ------------------------------------------------------------------------------------------ 7. determinism, size, errors
def test_determinism_and_batch_size():
    sh, batch, params, masks = problem("SMALL")
    hop_w, mw = [3, 3, 3], [0.7, 1.3]
    m = make_model(sh, params, masks)
    put(m, batch)
    first = step(m, hop_w, mw)
    same_bits(step(m, hop_w, mw), first)
    # n = 5 in the capacity-8 context against a context created at 5
    n = 5
    sh5 = dataclasses.replace(sh, B=n)
    b5 = {"feats": batch["feats"][:n], "tokens": np.ascontiguousarray(batch["tokens"][:, :n]),
          "lens": batch["lens"][:n], "labels": batch["labels"][:n]}
    m5k = {k: np.ascontiguousarray(v[:, :n]) for k, v in masks.items()}
    m.set_batch_size(n)
    m.set_masks(m5k)
    put(m, b5)
    got = step(m, hop_w, mw)
    gate = merge_ref.first_fire(m.dopred())
    m.close()
    assert 0 < gate.sum() < n                              # the select term is at work at this size, too
    m5 = make_model(sh5, params, m5k)
    put(m5, b5)
    same_bits(step(m5, hop_w, mw), got)
    m5.close()


def test_refusals():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    lib, h = m._lib, m._h
    args = (batch["feats"], batch["tokens"], batch["lens"])
    hop_w, mw = f32([3, 3, 3]), f32([0.7, 1.3])
    hp, mp = hop_w.ctypes.data, mw.ctypes.data
    m.set_batch(*args, batch["labels"])
    base = step(m, hop_w, None, how="plain")
    first = step(m, hop_w, mw)

    def launches():
        m.sync()
        return sum(v["launches"] for v in m.prof().values())

    def plain_still_works():
        m.set_batch(*args, batch["labels"])
        same_bits(step(m, hop_w, None, how="plain"), base)

    # a batch without labels: nothing launched
    m.set_batch(*args, None)
    m.forward()
    m.prof_enable()
    m.prof_reset()
    assert lib.rau_backward_merged(h, hp, None, None, mp) == STATE
    assert launches() == 0
    m.prof_enable(False)
    assert lib.rau_graph_step_merged(h, hp, None, None, mp, 1) == STATE
    plain_still_works()
    # the slot that forward read has been uploaded into since
    m.set_batch(*args, batch["labels"])
    m.forward()
    m.set_batch(*args, batch["labels"])
    m.prof_enable()
    m.prof_reset()
    assert lib.rau_backward_merged(h, hp, None, None, mp) == STATE
    assert launches() == 0
    m.prof_enable(False)
    plain_still_works()
    # non-finite weights
    m.set_batch(*args, batch["labels"])
    m.forward()
    for bad_w in (f32([np.nan, 1.3]), f32([0.7, np.inf])):
        assert lib.rau_backward_merged(h, hp, None, None, bad_w.ctypes.data) == INVALID
        assert lib.rau_graph_step_merged(h, hp, None, None, bad_w.ctypes.data, 1) == INVALID
    assert lib.rau_backward_merged(h, f32([3, np.nan, 3]).ctypes.data, None, None, mp) == INVALID
    assert lib.rau_merge_criterion_backward(h, None, None, None, mp, None) == INVALID
    plain_still_works()
    # one backward per forward holds for the new entry point too
    m.zero_grads()
    m.forward()
    assert lib.rau_backward_merged(h, hp, None, None, mp) == 0
    assert lib.rau_backward_merged(h, hp, None, None, mp) == STATE
    same_bits(m.get_grads(), first)
    plain_still_works()
    m.close()
