"""Answer vocabularies of any size on the GPU: K % 4 != 0 through the step path (rau_logits_pitch).

rau_create takes every K >= 2.  Where K % 4 != 0 the rows of logits, dl and the merged rows lie at the pitch
Kp = K rounded up to a multiple of 4 with +0 in the pad columns; everything the host reads stays dense in K, the
gradient rau_backward_ext takes stays dense [H,n,K], and the module-level calls that exchange [B,K] rows are refused.

The problems: util.make_problem at util.SMALL (H = 3) with K replaced, unless a case says otherwise.  Every problem
goes through vocab_problem(), which puts the labels of every third row at K itself (the last answer, inside the ragged
quad) and raises the classifier bias of answer K to the middle of the fp64 oracle's hop-0..H-1 gaps
(max_k<K logit - logit_K), so that about half of the rows have their first maximum at K; answer sets name K as well.
The logits feed nothing but the heads, so the bias moves no other quantity.

Bars.  f32: TOL = 1e-4 per layer slice (tests/test_gpu_select.py's, imported).  Integer results are exact wherever
the fp64 reference decides them (util.argmax_margin_ok).  bf16 mode: the derived bar and the nudged runs of
tests/test_gpu_bf16.run, which is called as it stands on vocab_problem()'s problem.  Bit-for-bit comparisons are
between two device runs, or against the numpy statements where the existing tests of those statements ask for bits.
"""
import ctypes as C
import dataclasses
import os
import socket
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from rau_vqa_amd import joint, predict
from tests import bce_ref, ext_ref, merge_ref, test_gpu_bf16, update_ref, util
from tests.test_gpu_ext import ext_step, linear_F, on_device, raw_ext, seeded_G
from tests.test_gpu_hop_merge import check_against_host
from tests.test_gpu_merged import step as merged_step
from tests.test_gpu_parity import run_gpu
from tests.test_gpu_select import GROUPS, INVALID, TOL, f32, grad_errs, make_model, same_bits, targets
from tests.test_gpu_topk import check_topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H3 = dict(util.SMALL, H=3)
REAL = dict(B=16, T=8, V=400, E=200, Rq=512, D=512, S=196, M=512, A=256, R=512, K=3129, H=2)
DP_DIMS = dict(util.SMALL, K=7, H=2)


# ------------------------------------------------------------------------------------------ problems
_PROBLEMS = {}


def cls_bias_offset(sh):
    """Offset of classifier.out_score.bias[K - 1] in the mult vector: behind it lie out_do_pred's M weights and 1 bias."""
    return oracle.group_sizes(sh)[2] - (sh.M + 1) - 1


def vocab_problem(dims, scale, seed=123, big_oracle=False):
    """(sh, batch, params, masks) with labels at K and answer K's bias raised (module docstring); computed once."""
    key = (tuple(sorted(dims.items())), scale, seed)
    if key not in _PROBLEMS:
        sh = util.shapes(dims)
        batch, params, masks = util.make_problem(sh, seed=seed, scale=scale)
        batch["labels"] = batch["labels"].copy()
        batch["labels"][::3] = sh.K
        step = RT.step if big_oracle else oracle.step
        fwd = step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks,
                   np.ones(sh.H, np.float32), backward=False, **({} if big_oracle else {"dtype": np.float64}))
        lg = np.asarray(fwd["logits"], np.float64)
        gaps = np.sort((lg[..., :-1].max(-1) - lg[..., -1]).ravel())
        mid = gaps.size // 2
        params = {k: v.copy() for k, v in params.items()}
        params["mult"][cls_bias_offset(sh)] += np.float32((gaps[mid - 1] + gaps[mid]) / 2)
        _PROBLEMS[key] = (sh, batch, params, masks)
    sh, batch, params, masks = _PROBLEMS[key]
    return sh, dict(batch), params, masks


def answer_set(sh, G=10, seed=7):
    """ids [B,G] with K itself in every third row, a duplicate, empty entries (some carrying a weight) and a row
    without entries; weights that do not sum to 1; scores with zeros among them."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, sh.K + 1, (sh.B, G)).astype(np.int32)
    ids[::3, 0] = sh.K
    ids[0, 1] = ids[0, 0]
    ids[1] = 0
    ids[2, 0], ids[2, 1] = 1, 0
    w = (rng.integers(1, 8, (sh.B, G)) / 8).astype(np.float32)
    score = np.minimum(rng.integers(0, 5, (sh.B, G)).astype(np.float32) / np.float32(3), np.float32(1))
    return ids, w, score.astype(np.float32)


def put(m, batch, **kw):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], **kw)


def assert_within(got, ref, layouts, what):
    errs = grad_errs(got, ref, layouts)
    worst = max(errs, key=errs.get)
    print(f"{what}: largest error {errs[worst]:.1e} ({worst})")
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"{what}: relative errors above {TOL}: {bad}"


def first_max_at_K(argmax, K):
    n = int((argmax == K).sum())
    assert 0 < n < argmax.size, f"{n} of {argmax.size} rows answer K: the bias does not split the rows"
    return n


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. parity
def parity(dims, scale, mode="train", big_oracle=False):
    sh, batch, params, masks = vocab_problem(dims, scale, big_oracle=big_oracle)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    mk = masks if mode == "train" else None
    if big_oracle:
        ref = RT.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], mk, hop_w)
    else:
        ref = oracle.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], mk, hop_w,
                          dtype=np.float64)
    got, layouts = run_gpu(sh, batch, params, masks, hop_w, mode)
    errs = {k: util.rel_err(got[k], ref[k]) for k in util.OUT_KEYS}
    errs.update(grad_errs({g: got["g_" + g] for g in GROUPS}, ref, layouts))
    worst = max(errs, key=errs.get)
    print(f"K={sh.K} {mode}: largest error {errs[worst]:.1e} ({worst})")
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"
    ok, decided, total = util.argmax_margin_ok(ref["logits"], got["argmax"], ref["argmax"])
    assert ok, "argmax mismatch on a decided row"
    if mode == "train":       # (the bias was placed under the train-mode masks)
        print(f"{first_max_at_K(got['argmax'], sh.K)} of {total} rows answer K; {decided} decided")
    return got, ref


@pytest.mark.parametrize("K", [2, 3, 5, 6, 7, 13])
def test_parity_in_train_mode(K):
    """Every remainder, and both sides of K = 4."""
    parity(dict(H3, K=K), 0.5)


def test_parity_medium_k1001():
    parity(dict(util.MEDIUM, K=1001), 0.2)


def test_parity_in_evaluate_mode():
    parity(dict(H3, K=7), 0.5, mode="eval")


# ------------------------------------------------------------------------------------------ 2. criteria
def test_answer_set_under_the_softmax_head():
    sh, batch, params, masks = vocab_problem(dict(H3, K=7), 0.5)
    ids, w, score = answer_set(sh)
    hop_w = [3, 3, 3]
    m = make_model(sh, params, masks)
    put(m, batch, answers=(ids, w, score))
    got = merged_step(m, hop_w, None, how="plain")
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = merge_ref.step(sh, params, batch, masks, hop_w, answers=(ids, w))
    assert_within(got, ref, layouts, "answer set, softmax")


@pytest.mark.parametrize("target", ["labels", "set"])
def test_sigmoid_head_against_bce_ref(target):
    sh, batch, params, masks = vocab_problem(dict(H3, K=7), 0.5)
    answers = answer_set(sh) if target == "set" else None
    hop_w = [3, 1, 2]
    m = make_model(sh, params, masks)
    m.set_answer_loss("bce")
    put(m, batch, **({} if answers is None else {"answers": answers}))
    got = merged_step(m, hop_w, None, how="plain")
    losses = m.losses()
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = bce_ref.step(sh, params, batch, masks, hop_w, answers=None if answers is None else answers[:2])
    assert util.rel_err(losses, ref["losses"]) < TOL
    assert_within(got, ref, layouts, f"sigmoid head, {target}")


def merged_parity(dims, scale, hop_w, merge_w, select_w=None):
    sh, batch, params, masks = vocab_problem(dims, scale)
    fwd = merge_ref.step(sh, params, batch, masks, [0.0] * sh.H, backward=False)
    m = make_model(sh, params, masks)
    put(m, batch)
    got = merged_step(m, hop_w, merge_w, select_w)
    assert np.array_equal(m.dopred() > 0.5, fwd["dopred"] > 0.5), "a do_pred crossed 0.5: choose another seed"
    hist = merge_ref.fire_histogram(merge_ref.first_fire(m.dopred()))
    t_gt = None
    if select_w is not None:
        am = m.argmax()
        ok, decided, total = util.argmax_margin_ok(fwd["logits"], am, fwd["argmax"])
        assert ok and decided == total, "an answer within the margin: choose another seed"
        t_gt = targets(am, batch)
        assert 0 < t_gt.sum() < t_gt.size
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = merge_ref.step(sh, params, batch, masks, hop_w, merge_w, select_w, t_gt)
    print(hist)
    assert_within(got, ref, layouts, f"merged K={sh.K}")
    return hist


def test_select_and_merged_terms_against_merge_ref():
    hist = merged_parity(dict(H3, K=7), 0.5, [3, 3, 3], [0.7, 1.3], [0.7, 0, 1.3])
    assert sum(v for k, v in hist.items() if k != "never") > 0, hist      # the select row is at work


@pytest.mark.parametrize("K", [4095, 4099])
def test_merged_terms_on_both_sides_of_the_staging_threshold(K):
    """What is staged is two rows at the pitch: 2 x 4096 floats fit the 32 KB, 2 x 4100 do not."""
    merged_parity(dict(H3, K=K), 0.5, [3, 3, 3], [0.7, 1.3])


def test_backward_ext_with_a_dense_d_logits():
    sh, batch, params, masks = vocab_problem(dict(H3, K=7), 0.5)
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    assert G["logits"].shape == (sh.H, sh.B, 7) and G["logits"].flags["C_CONTIGUOUS"]
    for labelled in (True, False):     # without labels the forward wrote no dl: dl = d_logits exactly
        b = batch if labelled else dict(batch, labels=None)
        m = make_model(sh, params, masks)
        m.set_batch(b["feats"], b["tokens"], b["lens"], b["labels"])
        got = ext_step(m, G, [3, 3, 3] if labelled else None)
        layouts = {k: m.layout(k) for k in GROUPS}
        m.close()
        ref = ext_ref.step(sh, params, b, masks, [3, 3, 3] if labelled else None, F=linear_F(G))
        assert_within(got, ref, layouts, f"ext, labelled={labelled}")


# ------------------------------------------------------------------------------------------ 3. bit identity
def test_selection_bce_stated_as_an_external_gradient_gives_the_same_bits():
    """tests/test_gpu_ext.py's statement at K = 7; with an all-zero dense d_logits beside it, which takes the ragged
    ext_dl pass in scale_hops' place (x w + 0: the same bits)."""
    sh, batch, params, masks = vocab_problem(dict(H3, K=7), 0.5)
    hop_w, select_w = [3, 0.5, 2], [0.7, 0, 1.3]
    m = make_model(sh, params, masks)
    put(m, batch)
    m.zero_grads()
    m.forward()
    hw, sw = f32(hop_w), f32(select_w)        # alive across the call
    L.check(m._lib.rau_backward_select(m._h, hw.ctypes.data, sw.ctypes.data))
    base = m.get_grads()
    for with_dl in (False, True):
        m.zero_grads()
        m.forward()
        t_gt = targets(m.argmax(), batch)
        assert 0 < t_gt.sum() < t_gt.size
        G = {"dopred": joint.bce_grad(m.dopred(), t_gt, f32(select_w))}
        if with_dl:
            G["logits"] = np.zeros((sh.H, sh.B, sh.K), np.float32)
        assert raw_ext(m, hop_w, None, None, None, on_device(G)) == 0
        same_bits(m.get_grads(), base)
    m.close()


# ------------------------------------------------------------------------------------------ 4. host-side results
@pytest.mark.parametrize("K", [7, 1001])
def test_host_side_results_against_the_numpy_statements(K):
    sh, batch, params, masks = vocab_problem(dict(H3, K=K), 0.5)
    H, B = sh.H, sh.B
    m = make_model(sh, params, masks)
    put(m, batch)
    m.forward()
    first_max_at_K(m.argmax(), K)
    lg = m.logits()
    assert lg.shape == (H, B, K)
    lt = m.output_tensors()[0]
    assert tuple(lt.shape) == (H, B, K) and np.array_equal(bits(lt.cpu().numpy()), bits(lg))
    check_against_host(m, batch["labels"])                       # rau_step_stats
    # rau_predict with an MC list that names answer K, against the host merges of the downloaded outputs
    rng = np.random.default_rng(2)
    mc = rng.integers(0, K + 1, size=(B, 6)).astype(np.int32)
    mc[:, 1] = 0
    mc[::2, 0] = K
    tab_pred, _ = predict.merge_hops(lg, m.dopred(), m.attention())
    oe, mco = m.predict(mc)
    want_oe = np.stack([np.argmax(t, axis=-1) + 1 for t in tab_pred])
    assert np.array_equal(oe, want_oe)
    cand = np.zeros((B, K), np.float32)
    for b in range(B):
        cand[b, mc[b][mc[b] > 0] - 1] = 1
    assert np.array_equal(mco, np.stack([np.argmax(t * cand, axis=-1) + 1 for t in tab_pred]))
    assert (mco == K).any()
    pred = m.merged()[0]                                         # rau_get_merged: dense [2,n,K] rows
    assert pred.shape == (2, B, K)
    assert np.array_equal(bits(pred[0]), bits(tab_pred[H])) and np.array_equal(bits(pred[1]), bits(tab_pred[H + 1]))
    for k in (K, 3):                                             # rau_topk
        ids, _score, _conf = check_topk(m, k, f"K{K}")
        if k == K:
            assert np.array_equal(np.sort(ids, axis=-1), np.broadcast_to(np.arange(1, K + 1), ids.shape))
    # rau_step_scores against the answer set
    ids, w, score = answer_set(sh)
    m.set_answers(ids, w, score)
    m.forward()
    per, _tot = m.step_scores()
    assert np.array_equal(per[:H], predict.answer_score(m.argmax(), ids, score))
    s = m.step_stats()
    ref = predict.set_stats(m.logits(), m.dopred(), ids, w, score)
    assert np.array_equal(s["loss"][:H], m.losses())
    assert util.rel_err(s["loss"], ref["loss"]) < TOL and np.array_equal(s["fired"], ref["fired"])
    m.close()


# ------------------------------------------------------------------------------------------ 5. pads
def raw_logits(m):
    """The whole pitched buffer behind output_tensors(): [H, n, pitch] on the host."""
    from rau_vqa_amd.dist import device_view
    lg = C.c_void_p()
    L.check(m._lib.rau_outputs_dev(m._h, C.byref(lg), None, None, None))
    H, n, kp = m.cfg.H, m.batch_size, m.logits_pitch
    m.sync()
    return device_view(lg.value, H * n * kp, m.cfg.device_id).view(H, n, kp).cpu().numpy()


def test_pitch_and_pad_columns():
    for K, pitch in ((7, 8), (12, 12)):
        sh, batch, params, masks = vocab_problem(dict(H3, K=K), 0.5)
        m = make_model(sh, params, masks)
        assert m.logits_pitch == pitch
        put(m, batch)
        m.zero_grads()
        m.forward()
        lt = m.output_tensors()[0]
        assert lt.stride() == (sh.B * pitch, pitch, 1) and tuple(lt.shape) == (sh.H, sh.B, K)
        raw = raw_logits(m)
        assert np.array_equal(bits(raw[..., :K]), bits(m.logits()))
        if pitch > K:
            assert not bits(raw[..., K:]).any(), "pad columns must hold +0 bits"
        m.backward(f32([3, 3, 3]), merge_w=[0.7, 1.3])
        m.sync()
        if pitch > K:
            assert not bits(raw_logits(m)[..., K:]).any()
        m.close()


def full_step(m, sh, batch, q=None):
    """A step with every pass that touches dl: select, merged and external terms; outputs, gradients, dq."""
    put(m, batch)
    if q is not None:
        m.set_question(q)
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    g = ext_step(m, G, [3, 1, 2], f32([0.7, 0, 1.3]), None, f32([0.7, 1.3]))
    out = [m.logits(), m.dopred(), m.losses(), m.argmax()] + [g[k] for k in GROUPS]
    if q is not None:
        out.append(m.question_grad())
    return out


def test_a_batch_with_huge_logits_leaves_nothing_behind():
    sh, batch_b, params, masks = vocab_problem(dict(H3, K=7), 0.5)
    _, batch_a, _, _ = vocab_problem(dict(H3, K=7), 0.5, seed=321)
    huge = {k: v.copy() for k, v in params.items()}
    off = cls_bias_offset(sh)
    huge["mult"][off - (sh.K - 1):off + 1] = 1000.0 * (1.0 + np.abs(huge["mult"][off - (sh.K - 1):off + 1]))
    q = torch.as_tensor(np.random.default_rng(4).normal(size=(sh.B, 4 * sh.Rq)).astype(np.float32) * 0.3).cuda()
    torch.cuda.synchronize()
    for attach in (None, q):
        m = make_model(sh, huge, masks)
        full_step(m, sh, batch_a, attach)
        assert np.abs(m.logits()).max() > 900
        m.set_params(params)
        got = full_step(m, sh, batch_b, attach)
        m.close()
        fresh = make_model(sh, params, masks)
        want = full_step(fresh, sh, batch_b, attach)
        fresh.close()
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b))


def test_no_extra_pass_for_the_pad():
    counts = {}
    for K in (12, 13):
        sh, batch, params, masks = vocab_problem(dict(H3, K=K), 0.5)
        m = make_model(sh, params, masks)
        put(m, batch)
        m.prof_enable()
        m.prof_reset()
        merged_step(m, [3, 3, 3], [0.7, 1.3])
        m.sync()
        counts[K] = {n: v["launches"] for n, v in m.prof().items() if v["launches"]}
        m.close()
    assert counts[12] == counts[13], (counts[12], counts[13])
    assert counts[13].get("merge_grad") == 1


# ------------------------------------------------------------------------------------------ 6. state
def test_graph_step_merged_replays_with_eager_bits():
    sh, batch, params, masks = vocab_problem(dict(H3, K=7), 0.5)
    m = make_model(sh, params, masks)
    put(m, batch)
    for mw in ([0.7, 1.3], [0.2, 2.0]):       # capture, then a replay at other values
        same_bits(merged_step(m, [3, 3, 3], mw, how="graph"), merged_step(m, [3, 3, 3], mw, how="merged"))
    m.close()


def test_a_resized_context_gives_the_bits_of_one_created_at_that_size():
    sh, batch, params, masks = vocab_problem(dict(H3, K=7), 0.5)
    n = 5
    sh5 = dataclasses.replace(sh, B=n)
    b5 = {"feats": batch["feats"][:n], "tokens": np.ascontiguousarray(batch["tokens"][:, :n]),
          "lens": batch["lens"][:n], "labels": batch["labels"][:n]}
    m5k = {k: np.ascontiguousarray(v[:, :n]) for k, v in masks.items()}
    m = make_model(sh, params, masks)
    put(m, batch)
    merged_step(m, [3, 3, 3], [0.7, 1.3])     # the full size first: what it leaves must not show
    m.set_batch_size(n)
    m.set_masks(m5k)
    put(m, b5)
    got = merged_step(m, [3, 3, 3], [0.7, 1.3])
    lg = m.logits()
    m.close()
    m5 = make_model(sh5, params, m5k)
    put(m5, b5)
    same_bits(merged_step(m5, [3, 3, 3], [0.7, 1.3]), got)
    assert np.array_equal(bits(m5.logits()), bits(lg))
    m5.close()


@pytest.mark.parametrize("rule,scope", [("adam", "group"), ("adamax", "global")])
def test_update_matches_update_ref(rule, scope):
    """The mult group's length and the offsets behind the classifier change parity with K.  Bar: 1e-5, the bar of
    tests/test_gpu_update_rules.py, for x, m, Adamax's u and the norms.  Adam's v gets 1e-5 + 2^-24 b2 / (1 - b2):
    the device forms (1 - b2) in float32 from b2 = 0.999f, whose rounding (up to 2^-24 b2) is that large a share
    of 1 - b2 = 0.001 -- a property of the number format, the same at every K (6.0e-5)."""
    sh, _batch, params, _masks = vocab_problem(dict(H3, K=7), 0.5)
    assert oracle.group_sizes(sh)[2] % 4 != 0
    rng = np.random.default_rng(3)
    m = make_model(sh, params)
    x = {k: v.astype(np.float64) for k, v in params.items()}
    mo = {k: np.zeros(v.size) for k, v in params.items()}
    vo = {k: np.zeros(v.size) for k, v in params.items()}
    for t in range(2):
        grads = {k: (rng.standard_normal(v.size) * 0.01).astype(np.float32) for k, v in params.items()}
        m.set_grads(grads)
        norms = m.update(step_t=t, lr=3e-3, mult_lr=3e-4, eta=0.0, clip=0.1, rule=rule, clip_scope=scope)
        x, _gc, mo, vo, ref_norms = update_ref.update(x, grads, mo, vo, {k: t + 1 for k in GROUPS}, t, rule=rule,
                                                      clip_scope=scope, eta=0.0, clip=0.1)
        got, (st, _rule) = m.get_params(), m.opt_state()
        v_bar = 1e-5 + (2.0 ** -24 * 0.999 / 0.001 if rule == "adam" else 0.0)
        for k in GROUPS:
            for name, a, b, bar in (("x", got[k], x[k], 1e-5), ("m", st[k][0], mo[k], 1e-5),
                                    ("v", st[k][1], vo[k], v_bar)):
                err = util.rel_err(a, b)
                print(f"{rule} {k}.{name}: {err:.2e} (bar {bar:.1e})")
                assert err < bar, (k, name, err)
        for i in range(len(norms)):
            assert abs(norms[i] - ref_norms[i]) < 1e-5 * max(1.0, ref_norms[i]), i
    m.close()


def test_snapshot_with_optimizer_state_round_trips(tmp_path):
    sh, _batch, params, _masks = vocab_problem(dict(H3, K=7), 0.5)
    rng = np.random.default_rng(5)
    a = make_model(sh, params)
    a.set_grads({k: (rng.standard_normal(v.size) * 0.01).astype(np.float32) for k, v in params.items()})
    a.update(step_t=0, eta=0.01, noise_seed=3, rule="adamax", clip_scope="global")
    path = str(tmp_path / "k7.t7")
    a.save_snapshot(path, 1, 0, {"lr": 3e-3}, optim=True)
    b = make_model(sh, {k: np.zeros_like(v) for k, v in params.items()})
    assert b.load_snapshot(path) == (1, 0, {"lr": 3e-3})
    pa, pb = a.get_params(), b.get_params()
    (sa, ra), (sb, rb) = a.opt_state(), b.opt_state()
    assert ra == rb == "adamax"
    for k in GROUPS:
        assert np.array_equal(bits(pa[k]), bits(pb[k])) and sa[k][2] == sb[k][2]
        assert np.array_equal(bits(sa[k][0]), bits(sb[k][0])) and np.array_equal(bits(sa[k][1]), bits(sb[k][1]))
    a.close()
    b.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from rau_vqa_amd.dist import GradAllReduce, shard_batch
    from rau_vqa_amd.model import RAU, Config
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sh = util.shapes(DP_DIMS)
    batch, params, _ = util.make_problem(sh, scale=0.5)
    m = RAU(Config(**dict(DP_DIMS, B=DP_DIMS["B"] // world)))
    m.set_params(params)
    m.evaluate()
    m.set_batch(**shard_batch(batch, rank, world))
    m.zero_grads()
    m.forward()
    m.backward(np.full(sh.H, float(sh.H), np.float32))
    GradAllReduce(m)()
    torch.cuda.synchronize()
    m.sync()
    q.put((rank, {k: v.copy() for k, v in m.get_grads().items()}))
    m.close()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_hold_identical_averaged_gradients():
    """tests/test_gpu_dp.py's flow at K = 7: three processes with the GPU open, this one included."""
    import torch.multiprocessing as mp
    from rau_vqa_amd.model import RAU, Config
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for k in GROUPS:
        assert np.array_equal(bits(got[0][k]), bits(got[1][k])), k
    sh = util.shapes(DP_DIMS)
    batch, params, _ = util.make_problem(sh, scale=0.5)
    m = RAU(Config(**DP_DIMS))
    m.set_params(params)
    m.evaluate()
    m.set_batch(**batch)
    m.zero_grads()
    m.forward()
    m.backward(np.full(sh.H, float(sh.H), np.float32))
    ref = m.get_grads()
    m.close()
    for k in ref:
        assert util.rel_err(got[0][k], ref[k]) < 1e-5, k


# ------------------------------------------------------------------------------------------ 7. refusals
def test_one_answer_is_refused():
    from rau_vqa_amd.model import RAU, Config
    with pytest.raises(L.RauError, match="at least two answers"):
        RAU(Config(**dict(H3, K=1)))


def module_calls(m, sh, dev):
    """Every module-level call that exchanges [B,K] rows, as (name, return code) in a fixed order."""
    lib, h = m._lib, m._h
    p = lambda t: C.c_void_p(t.data_ptr())
    outs = [C.c_void_p() for _ in range(5)]
    refs = [C.byref(o) for o in outs]
    loss, o1 = C.c_float(), C.c_void_p()
    mw = f32([0.7, 1.3])
    q, lg, y, ids, w, lgs, dps, dls, reg = (dev[k] for k in ("q", "lg", "y", "ids", "w", "lgs", "dps", "dls", "reg"))
    G = ids.shape[1]
    calls = [
        ("rau_multimodal_forward", lambda: lib.rau_multimodal_forward(h, 0, p(q), None, None, None, *refs)),
        ("rau_multimodal_forward_regions",
         lambda: lib.rau_multimodal_forward_regions(h, 0, p(q), None, None, None, p(reg), *refs)),
        ("rau_multimodal_backward",
         lambda: lib.rau_multimodal_backward(h, 0, p(q), None, None, None, p(lg), None, None, None, None, *refs[:4])),
        ("rau_criterion_forward", lambda: lib.rau_criterion_forward(h, 0, p(lg), p(y), C.byref(loss))),
        ("rau_criterion_backward", lambda: lib.rau_criterion_backward(h, 0, p(lg), p(y), 1.0, C.byref(o1))),
        ("rau_criterion_forward_set", lambda: lib.rau_criterion_forward_set(h, 0, p(lg), G, p(ids), p(w), C.byref(loss))),
        ("rau_criterion_backward_set",
         lambda: lib.rau_criterion_backward_set(h, 0, p(lg), G, p(ids), p(w), 1.0, C.byref(o1))),
        ("rau_criterion_forward_bce",
         lambda: lib.rau_criterion_forward_bce(h, 0, p(lg), p(y), 0, None, None, C.byref(loss))),
        ("rau_criterion_backward_bce",
         lambda: lib.rau_criterion_backward_bce(h, 0, p(lg), p(y), 0, None, None, 1.0, C.byref(o1))),
        ("rau_merge_criterion_backward",
         lambda: lib.rau_merge_criterion_backward(h, p(lgs), p(dps), p(y), mw.ctypes.data, p(dls))),
    ]
    return [(name, fn()) for name, fn in calls]


@pytest.mark.parametrize("K", [7, 12])
def test_module_level_calls_are_refused_where_k_is_ragged_and_work_where_it_is_not(K):
    from rau_vqa_amd import modules
    sh, batch, params, masks = vocab_problem(dict(H3, K=K), 0.5)
    m = make_model(sh, params, masks)
    put(m, batch)
    base = merged_step(m, [3, 3, 3], [0.7, 1.3])
    rng = np.random.default_rng(1)
    ids, w, _ = answer_set(sh, G=3)
    host = {"q": rng.normal(size=(sh.B, 4 * sh.Rq)) * 0.3, "lg": rng.normal(size=(sh.B, K)),
            "lgs": rng.normal(size=(sh.H, sh.B, K)), "dps": rng.uniform(size=(sh.H, sh.B)),
            "dls": np.zeros((sh.H, sh.B, K)), "w": w}
    dev = {k: torch.as_tensor(np.ascontiguousarray(v, np.float32)).cuda() for k, v in host.items()}
    dev["y"] = torch.as_tensor(batch["labels"].astype(np.int32)).cuda()
    dev["ids"] = torch.as_tensor(ids).cuda()
    dev["reg"] = torch.full((sh.B,), sh.S, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    put(m, batch)
    m.prof_enable()
    m.prof_reset()
    rcs = module_calls(m, sh, dev)
    m.sync()
    launches = sum(v["launches"] for v in m.prof().values())
    m.prof_enable(False)
    cuda = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).cuda().to(dt)
    feval_args = (m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32), cuda(batch["lens"], torch.int32),
                  dev["y"], f32([3, 3, 3]))
    if K % 4:
        assert all(rc == INVALID for _name, rc in rcs), rcs
        assert "K % 4 == 0" in m._lib.rau_last_error().decode()
        assert launches == 0
        with pytest.raises(L.RauError, match="K % 4 == 0"):
            modules.feval(*feval_args)
    else:
        assert all(rc == 0 for _name, rc in rcs), rcs
        assert launches > 0
        m.zero_grads()
        modules.feval(*feval_args)
        m.sync()
    # the context is as usable as before: the same step, the same bits
    m.set_masks(masks)
    put(m, batch)
    same_bits(merged_step(m, [3, 3, 3], [0.7, 1.3]), base)
    m.close()


# ------------------------------------------------------------------------------------------ 8. bf16 mode
def run_bf16(monkeypatch, dims, scale, big_oracle=False):
    """tests/test_gpu_bf16.run as it stands -- the emulating oracle, its nudged runs, the derived bar, the exact-oracle
    bar, the answer indices -- on vocab_problem()'s problem."""
    problem = vocab_problem(dims, scale, big_oracle=big_oracle)
    sh = problem[0]

    def make_problem(sh_, **_kw):
        assert dataclasses.asdict(sh_) == dataclasses.asdict(sh)
        return dict(problem[1]), problem[2], problem[3]
    monkeypatch.setattr(util, "make_problem", make_problem)
    test_gpu_bf16.run(dims, scale)


@pytest.mark.parametrize("K", [7, 1001])
def test_bf16_mode_against_the_emulating_oracle(monkeypatch, K):
    dims = dict(H3, K=7) if K == 7 else dict(util.MEDIUM, K=1001)
    run_bf16(monkeypatch, dims, 0.5 if K == 7 else 0.2)


# ------------------------------------------------------------------------------------------ 9. real widths
def test_real_widths_k3129_f32():
    got, ref = parity(REAL, 0.05, big_oracle=True)
    ok, decided, total = util.argmax_margin_ok(ref["logits"], got["argmax"], ref["argmax"])
    assert ok and decided > 0


def test_real_widths_k3129_bf16(monkeypatch):
    run_bf16(monkeypatch, REAL, 0.05, big_oracle=True)
