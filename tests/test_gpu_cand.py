"""Multiple-choice candidates on the GPU (rau_set_candidates, cand_head.hip, cand_rank.hip): the criterion head
restricted to a sample's candidates, the ranked MC answers and the MC statistics.

The fp64 whole-step reference is tests/cand_ref.py (tests/ext_ref.step with the restricted criterion as its callable
F, on the unchanged oracle); the machinery is tests/test_gpu_select.py's and tests/test_gpu_sample_weights.py's: the
committed problems under their explicit masks, make_model, grad_errs, same_bits, TOL = 1e-4 per layer slice, and in bf16
mode the bar tests/test_gpu_bf16.py derives.  The candidate lists (candidates() below) hold every row class in one
batch: 0 plain, 1 duplicates, 2 empties, 3 truth outside the list, 4 no live candidate, 5 a single candidate that is
its truth, 6.. plain.

The pad of dl at K = 13 has no getter of its own (the module-level calls need K % 4 == 0): the row clear that writes
it is checked bit for bit on dense rows in the contract test, and at K = 13 a pad that were not zero would enter the
classifier's gradients, which the parity case bounds."""
import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from rau_vqa_amd import joint, modules, predict
from tests import att_ref, cand_ref, ext_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_ext import COUNTS8, ext_step, linear_F, seeded_G
from tests.test_gpu_merged import step as merged_step
from tests.test_gpu_modules import cuda
from tests.test_gpu_sample_weights import assert_within, forward_ref, gates_agree, weights
from tests.test_gpu_select import (GROUPS, INVALID, STATE, TOL, f32, make_model, problem, same_bits,
                                   small_answer_set)

pytestmark = pytest.mark.gpu

HOP_W = [3, 0.5, 2]


# ------------------------------------------------------------------------------------------ machinery
def candidates(sh, truth, C=5, seed=11):
    """cand [B, C] int32 around the 1-based truth ids `truth` [B] (0: the row has none), with the row classes of the
    module docstring (B >= 6)."""
    rng = np.random.default_rng(seed)
    cand = np.zeros((sh.B, C), np.int32)
    for b in range(sh.B):
        y = int(truth[b]) if truth[b] > 0 else 1
        others = rng.permutation([k for k in range(1, sh.K + 1) if k != y])[:C - 1]
        cand[b] = np.concatenate([[y], others])[rng.permutation(C)]
    y = [int(t) if t > 0 else 1 for t in truth]
    o = lambda b, i: [k for k in range(1, sh.K + 1) if k != y[b]][i]
    cand[1] = ([y[1], o(1, 0), y[1], o(1, 0), o(1, 1)] + [y[1]] * C)[:C]
    cand[2] = ([0, y[2], 0, o(2, 2), 0] + [0] * C)[:C]
    cand[3] = [o(3, i) for i in range(C)] if sh.K > C else 0
    cand[4] = 0
    cand[5] = ([0, 0, y[5]] + [0] * C)[:C]
    return cand


def put(m, batch, **kw):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], **kw)


def dev_step(m, hop_w, select_w=None, att_w=None, how="merged"):
    return merged_step(m, hop_w, None, select_w, att_w, how=how)


def check_rows(m, ref, what):
    rows, losses = m.loss_rows(), m.losses()
    print(f"{what}: rows {util.rel_err(rows, ref['rows']):.1e} losses {util.rel_err(losses, ref['rows'].mean(1)):.1e}")
    assert util.rel_err(rows, ref["rows"]) < TOL and util.rel_err(losses, ref["rows"].mean(1)) < TOL
    return rows


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("target,evaluate,weighted", [
    ("labels", False, False), ("set", False, True), ("labels", True, True), ("set", True, False),
    ("bce_labels", False, True), ("bce_set", False, False), ("bce_set", True, True)])
def test_parity_small(target, evaluate, weighted):
    sh, batch, params, masks = problem("SMALL")
    answers = small_answer_set(batch, sh) if target.endswith("set") else None
    loss = "bce" if target.startswith("bce") else "ce"
    cand = candidates(sh, batch["labels"] if answers is None else answers[0][:, 0])
    s = weights(sh.B) if weighted else None
    masks = None if evaluate else masks
    m = make_model(sh, params, masks)
    if evaluate:
        m.evaluate()
    m.set_answer_loss(loss)
    kw = {} if answers is None else {"answers": answers}
    put(m, batch, candidates=cand, sample_w=s, **kw)
    assert m.batch_candidates == 5
    got = dev_step(m, HOP_W)
    layouts = {k: m.layout(k) for k in GROUPS}
    ref = cand_ref.step(sh, params, batch, masks, cand, HOP_W, s, answers, loss)
    rows = check_rows(m, ref, target)
    argmax, logits = m.argmax(), m.logits()
    m.close()
    assert_within(got, ref, layouts, target)
    assert np.array_equal(argmax, np.argmax(logits, -1) + 1)            # the open-ended answer: over all K
    assert np.all(rows[:, 4] == 0)                                      # no live candidate
    if target.endswith("labels"):
        assert np.all(rows[:, 3] == 0)                                  # the truth outside the list
    if target == "labels":
        assert np.abs(rows[:, 5]).max() < 1e-6                          # the one live candidate is the truth
        assert rows[:, 0].min() > 1e-3
    if target == "labels" and not evaluate:   # the candidates are at work in the oracle: ignoring them cannot pass
        plain = ext_ref.step(sh, params, batch, masks, HOP_W)
        diff = [util.rel_err(ref["g_" + k], plain["g_" + k]) for k in GROUPS]
        print("restricted vs full-vocabulary oracle:", diff)
        assert min(diff) > 0.05


def class_parity(sh, batch, params, masks, cand, hop_w, what):
    m = make_model(sh, params, masks)
    put(m, batch, candidates=cand)
    got = dev_step(m, hop_w)
    layouts = {k: m.layout(k) for k in GROUPS}
    ref = cand_ref.step(sh, params, batch, masks, cand, hop_w)
    check_rows(m, ref, what)
    m.close()
    assert_within(got, ref, layouts, what)


def test_parity_pitched_rows_K13():
    sh = util.shapes(util.SMALL, K=13)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    class_parity(sh, batch, params, masks, candidates(sh, batch["labels"]), HOP_W, "K = 13")


def test_parity_medium_C32_partials_finished_inside_the_head():
    sh, batch, params, masks = problem("MEDIUM")
    class_parity(sh, batch, params, masks, candidates(sh, batch["labels"], C=32), [2, 2], "MEDIUM C = 32")


def test_parity_edge():
    sh, batch, params, masks = problem("EDGE")
    cand = np.array([[batch["labels"][b], b % sh.K + 1, 0] for b in range(sh.B)], np.int32)
    class_parity(sh, batch, params, masks, cand, [1], "EDGE")


def test_bf16_mode_against_the_emulated_oracle():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])
    m = make_model(sh, params, masks, dtype="bf16")
    put(m, batch, candidates=cand)
    got = dev_step(m, HOP_W)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    with RT.bf16_emulation():
        emu = cand_ref.step(sh, params, batch, masks, cand, HOP_W, bf16=True)
    nudged = []
    for n in NUDGES:
        with RT.bf16_emulation(n):
            nudged.append(cand_ref.step(sh, params, batch, masks, cand, HOP_W, bf16=True))
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
    print(f"bf16 candidates: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated oracle, (error, derived bar): {bad}"


# ------------------------------------------------------------------------------------------ 2. the kernel's contract
@pytest.mark.parametrize("K", [12, 2052])
@pytest.mark.parametrize("kind", ["ce", "bce"])
def test_module_level_contract(kind, K):
    sh = util.shapes(util.SMALL, K=K)
    _batch, params, _masks = util.make_problem(sh, scale=0.5)
    m = make_model(sh, params)
    rng = np.random.default_rng(K)
    x = (rng.normal(size=(sh.B, K)) * 3).astype(np.float32)
    x[6] = np.where(rng.uniform(size=K) < 0.5, 80.0, -80.0)             # saturated logits stay finite
    y = rng.integers(1, K + 1, size=sh.B).astype(np.int32)
    C = 32 if K > 32 else 5
    cand = candidates(sh, y, C=C)
    ids = np.stack([y, rng.integers(0, K + 1, size=sh.B), y], 1).astype(np.int32)
    w = rng.uniform(0.1, 1.0, size=ids.shape).astype(np.float32)
    crit = modules.CandCriterionClone(m, 1)
    fwd, bwd = (predict.cand_ce, predict.cand_ce_grad) if kind == "ce" else (predict.cand_bce, predict.cand_bce_grad)
    xd, yd, cd = cuda(x), cuda(y, torch.int32), cuda(cand, torch.int32)
    ans = (cuda(ids, torch.int32), cuda(w))
    torch.cuda.synchronize()
    live = np.zeros((sh.B, K), bool)
    for b in range(sh.B):
        live[b, [c - 1 for c in cand[b] if c > 0]] = True
    for what, yy, aa, ii, ww in (("labels", yd, None, y, None), ("set", None, ans, ids, w)):
        loss = crit.forward(xd, yy, cd, aa, kind)
        g = crit.backward(xd, yy, cd, aa, kind, 2.0)
        m.sync()
        g = g.cpu().numpy()
        want_rows, want_loss = fwd(x, cand, ii, ww)
        want = np.float32(2) * bwd(x, cand, ii, ww)
        den = max(np.max(np.abs(want)), 1e-30)
        print(kind, K, what, abs(loss - want_loss), np.max(np.abs(g - want)) / den)
        assert abs(loss - want_loss) < 1e-6 * max(1.0, abs(want_loss))
        assert np.max(np.abs(g - want)) / den < 1e-6
        assert np.isfinite(g).all() and np.isfinite(loss)
        assert not bits(g)[~live].any()                                  # +0 bits outside the live candidates
        assert not bits(g)[3].any() and not bits(g)[4].any()             # unlabelled rows
        assert want_rows[3] == 0 and want_rows[4] == 0
        again = crit.backward(xd, yy, cd, aa, kind, 2.0)
        m.sync()
        assert np.array_equal(bits(again.cpu().numpy()), bits(g))        # the same bits on every call
    none = cuda(np.zeros_like(cand), torch.int32)                        # every row unlabelled: loss 0, +0 bits
    torch.cuda.synchronize()
    assert crit.forward(xd, yd, none, None, kind) == 0.0
    g0 = crit.backward(xd, yd, none, None, kind)
    m.sync()
    assert not bits(g0.cpu().numpy()).any()
    lib, h = m._lib, m._h
    o, lo = L.C.c_void_p(), L.C.c_float()
    p = lambda t: L.C.c_void_p(t.data_ptr())
    assert lib.rau_criterion_forward_cand(h, 0, p(xd), p(yd), 0, None, None, 0, p(cd), 0, L.C.byref(lo)) == INVALID
    assert lib.rau_criterion_forward_cand(h, 0, p(xd), p(yd), 0, None, None, 33, p(cd), 0, L.C.byref(lo)) == INVALID
    assert lib.rau_criterion_forward_cand(h, 0, p(xd), p(yd), 0, None, None, C, None, 0, L.C.byref(lo)) == INVALID
    assert lib.rau_criterion_forward_cand(h, 0, p(xd), None, 0, None, None, C, p(cd), 0, L.C.byref(lo)) == INVALID
    assert lib.rau_criterion_backward_cand(h, 0, p(xd), p(yd), 0, None, None, C, p(cd), 2, 1.0, L.C.byref(o)) == INVALID
    assert lib.rau_criterion_backward_cand(h, sh.H, p(xd), p(yd), 0, None, None, C, p(cd), 0, 1.0, L.C.byref(o)) == INVALID
    m.close()


# ------------------------------------------------------------------------------------------ 3. unchanged without
def test_a_batch_without_candidates_is_untouched_bit_for_bit_and_launch_for_launch():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])

    def run(m):
        m.prof_reset()
        g = dev_step(m, HOP_W)
        m.sync()
        listing = {n: v["launches"] for n, v in m.prof().items() if v["launches"]}
        return g, listing, m.logits(), m.losses(), m.loss_rows()

    a = make_model(sh, params, masks)
    a.prof_enable()
    put(a, batch, candidates=cand)
    with_c = run(a)
    assert with_c[1].get("cand_fwd", 0) > 0 and "ce_fwd" not in with_c[1]
    put(a, batch)                                        # the next batch comes without them
    assert a.batch_candidates == 0
    after = run(a)
    b = make_model(sh, params, masks)
    b.prof_enable()
    put(b, batch)
    never = run(b)
    same_bits(after[0], never[0])
    for x, y in zip(after[2:], never[2:]):
        assert np.array_equal(bits(x), bits(y))
    assert after[1] == never[1] and "cand_fwd" not in after[1] and after[1]["ce_fwd"] == with_c[1]["cand_fwd"]
    assert {k: v for k, v in with_c[1].items() if k != "cand_fwd"} == {k: v for k, v in never[1].items() if k != "ce_fwd"}
    assert any(not np.array_equal(with_c[0][k], never[0][k]) for k in GROUPS)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------ 4. ranks and statistics
@pytest.mark.parametrize("target", ["labels", "set", "bce_set"])
def test_ranked_candidates_and_statistics(target):
    sh, batch, params, masks = problem("SMALL")
    answers = small_answer_set(batch, sh) if target.endswith("set") else None
    loss = "bce" if target.startswith("bce") else "ce"
    cand = candidates(sh, batch["labels"] if answers is None else answers[0][:, 0], C=6)
    cand[7, 5] = cand[7, 0]                               # a duplicate behind the live entries
    s = weights(sh.B)
    m = make_model(sh, params)
    m.evaluate()
    m.set_answer_loss(loss)
    put(m, batch, candidates=cand, sample_w=s, **({} if answers is None else {"answers": answers}))
    m.forward()
    logits, dopred, att = m.logits(), m.dopred(), m.attention()
    tab_pred, _ = predict.merge_hops(logits, dopred, att)             # predict rule: the last hop forced
    for k in (1, 3, 6):
        ids, score, conf = m.top_candidates(k)
        w_ids, w_score, w_conf = predict.top_candidates(tab_pred, cand, k)
        assert np.array_equal(ids, w_ids) and np.array_equal(bits(score), bits(w_score))
        assert np.max(np.abs(conf - w_conf)) < 1e-6
    assert np.all(ids[:, 4] == 0) and np.all(np.isneginf(score[:, 4])) and not bits(conf[:, 4]).any()
    assert np.all(ids[:, 5, 1:] == 0) and np.all(conf[:, 5, 0] == 1)
    assert abs(conf[:, 0].sum(-1) - 1).max() < 1e-5
    oe, mc = m.predict(cand)
    pos = score[:, :, 0] > 0
    assert pos.any() and np.array_equal(mc[pos], ids[:, :, 0][pos])    # the multiply rule where the best is positive
    assert np.array_equal(m.topk(1)[0][:, :, 0], oe)                   # the open-ended calls: untouched
    st = m.cand_stats()
    if answers is None:
        want = predict.cand_stats(logits, dopred, cand, batch["labels"], loss=loss, sample_w=s)
        plain = joint.feval_stats(logits, dopred, batch["labels"], sample_w=s)
    else:
        want = predict.cand_stats(logits, dopred, cand, *answers, loss=loss, sample_w=s)
        plain = predict.set_stats(logits, dopred, *answers, loss=loss, sample_w=s)
    assert np.array_equal(bits(st["loss"][:sh.H]), bits(m.losses()))  # bitwise rau_get_losses
    print(target, st, want["loss"])
    assert util.rel_err(st["loss"][sh.H:], want["loss"][sh.H:]) < 1e-5
    assert util.rel_err(st["loss"][:sh.H], want["loss"][:sh.H]) < 1e-5
    assert np.array_equal(st["correct"], want["correct"]) and np.array_equal(bits(st["score"]), bits(want["score"]))
    assert st["n_lab"] == want["n_lab"]
    again = m.cand_stats()
    assert all(np.array_equal(again[k], st[k]) for k in st)
    full = m.step_stats()                                               # its loss[:H] are the restricted rows ...
    assert np.array_equal(bits(full["loss"][:sh.H]), bits(m.losses()))
    for k in ("correct", "fired", "selected"):                          # ... everything else stays open-ended
        assert np.array_equal(full[k], plain[k]), k
    assert util.rel_err(full["loss"][sh.H:], plain["loss"][sh.H:]) < 1e-4
    m.close()


# ------------------------------------------------------------------------------------------ 5. state and errors
def raw_set(m, slot, cand):
    if cand is None:
        return m._lib.rau_set_candidates(m._h, slot, 0, None)
    cand = np.ascontiguousarray(cand, np.int32)
    return m._lib.rau_set_candidates(m._h, slot, cand.shape[1], cand.ctypes.data)


def test_state_slots_and_errors():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])
    m = make_model(sh, params, masks)
    assert raw_set(m, -1, cand) == STATE and raw_set(m, 0, cand) == STATE     # no batch anywhere yet
    put(m, batch)
    plain = dev_step(m, HOP_W)
    assert m._lib.rau_topk_cand(m._h, 1, None, None, None) == STATE           # a forward, but no candidates
    assert m._lib.rau_cand_stats(m._h, None, None, None, None) == STATE
    m.set_candidates(cand)
    assert m._lib.rau_topk_cand(m._h, 1, None, None, None) == STATE           # the forward must be rerun
    want = dev_step(m, HOP_W)
    rows = m.loss_rows()
    assert any(not np.array_equal(want[k], plain[k]) for k in GROUPS)
    # errors leave the previous list in force
    for bad in (np.full((sh.B, 5), sh.K + 1), np.full((sh.B, 5), -1)):
        assert raw_set(m, -1, bad) == INVALID
    assert m._lib.rau_set_candidates(m._h, -1, 33, np.zeros((sh.B, 33), np.int32).ctypes.data) == INVALID
    assert m._lib.rau_set_candidates(m._h, -1, -1, cand.ctypes.data) == INVALID
    assert raw_set(m, 2, cand) == INVALID
    assert m.batch_candidates == 5
    same_bits(dev_step(m, HOP_W), want)
    for k_bad in (0, 6):
        assert m._lib.rau_topk_cand(m._h, k_bad, None, None, None) == INVALID
    assert m._lib.rau_topk_cand(m._h, 5, None, None, None) == 0
    # a non-zero merge_w is refused, the gradients stay, the forward stays usable
    m.zero_grads()
    m.forward()
    g0 = m.get_grads()
    hw, mw = f32(HOP_W), f32([0.7, 1.3])
    assert m._lib.rau_backward_merged(m._h, hw.ctypes.data, None, None, mw.ctypes.data) == INVALID
    assert m._lib.rau_graph_step_merged(m._h, hw.ctypes.data, None, None, mw.ctypes.data, 1) == INVALID
    assert m._lib.rau_backward_ext(m._h, hw.ctypes.data, None, None, mw.ctypes.data, None) == INVALID
    same_bits(m.get_grads(), g0)
    zeros = f32([0, 0])
    L.check(m._lib.rau_backward_merged(m._h, hw.ctypes.data, None, None, zeros.ctypes.data))   # zeros: the path without
    same_bits(m.get_grads(), want)
    # detach by NULL; the forward must be rerun
    m.forward()
    assert raw_set(m, -1, None) == 0 and m.batch_candidates == 0
    with pytest.raises(L.RauError):
        m.backward(f32(HOP_W))
    same_bits(dev_step(m, HOP_W), plain)
    assert raw_set(m, -1, None) == 0
    # cleared by an upload and by rau_set_batch_size
    m.set_candidates(cand)
    put(m, batch)
    assert m.batch_candidates == 0
    same_bits(dev_step(m, HOP_W), plain)
    m.set_candidates(cand)
    m.set_batch_size(5)
    assert raw_set(m, -1, cand[:5]) == STATE
    m.set_batch_size(sh.B)
    m.set_masks(masks)
    put(m, batch)
    assert m.batch_candidates == 0
    same_bits(dev_step(m, HOP_W), plain)
    # the asynchronous path, both slots
    up = lambda slot, **kw: m.set_batch_async(slot, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], **kw)
    assert raw_set(m, 1, cand) == STATE                  # slot 1 holds no batch
    up(1)
    m.set_candidates(cand, slot=1)
    assert m.batch_candidates == 0                       # slot 0 is still the resident batch
    m.use_batch(1)
    assert m.batch_candidates == 5
    same_bits(dev_step(m, HOP_W), want)
    assert np.array_equal(m.loss_rows(), rows)
    up(0)                                                # the other slot: left alone
    assert m.batch_candidates == 5
    m.use_batch(0)
    assert m.batch_candidates == 0
    same_bits(dev_step(m, HOP_W), plain)
    up(1, candidates=cand)
    up(1)                                                # a later upload clears them
    m.use_batch(1)
    assert m.batch_candidates == 0
    up(0, candidates=cand)
    m.use_batch(0)
    assert m.batch_candidates == 5
    same_bits(dev_step(m, HOP_W), want)
    m.forward()
    assert raw_set(m, 0, cand) == STATE                  # the current batch of a forward whose backward has not run
    assert raw_set(m, -1, cand) == 0                     # the resident form may: the forward is dropped
    m.close()


# ------------------------------------------------------------------------------------------ 6. captured steps
def test_graph_step_with_candidates():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])
    cand2 = candidates(sh, batch["labels"], seed=12)
    assert not np.array_equal(cand, cand2)
    m = make_model(sh, params, masks)
    put(m, batch)
    plain = dev_step(m, HOP_W)
    same_bits(dev_step(m, HOP_W, how="graph"), plain)    # captured without candidates
    m.set_candidates(cand)
    eager = dev_step(m, HOP_W)
    rows = m.loss_rows()
    same_bits(dev_step(m, HOP_W, how="graph"), eager)    # another graph
    assert np.array_equal(m.loss_rows(), rows)
    same_bits(dev_step(m, HOP_W, how="graph"), eager)    # the replay
    m.set_candidates(cand2)                              # same C, new contents: the replay reads the current list
    eager2 = dev_step(m, HOP_W)
    assert any(not np.array_equal(eager2[k], eager[k]) for k in GROUPS)
    same_bits(dev_step(m, HOP_W, how="graph"), eager2)
    m.set_candidates(cand[:, :4])                        # another C: not a replay of the old graph
    eager4 = dev_step(m, HOP_W)
    same_bits(dev_step(m, HOP_W, how="graph"), eager4)
    m.clear_candidates()
    same_bits(dev_step(m, HOP_W, how="graph"), plain)    # none: the first graph again
    m.set_candidates(cand)
    same_bits(dev_step(m, HOP_W, how="graph"), eager)
    m.close()


# ------------------------------------------------------------------------------------------ 7. together
def test_with_select_att_targets_and_region_counts():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])
    select_w, att_w = [0.7, 0.4, 1.3], [0.5, 3.0, 1.5]
    fwd = forward_ref(sh, params, batch, masks, COUNTS8)
    t = att_ref.targets(fwd["att"], COUNTS8)
    m = make_model(sh, params, masks)
    put(m, batch, candidates=cand, regions=COUNTS8, att_targets=t)
    got = dev_step(m, HOP_W, select_w, att_w)
    t_gt = gates_agree(m, fwd)                           # do_pred_gt stays the open-ended argmax == y
    layouts = {k: m.layout(k) for k in GROUPS}
    ref = cand_ref.step(sh, params, batch, masks, cand, HOP_W, select_w=select_w, t_gt=t_gt, att_w=att_w, att_t=t,
                        nreg=COUNTS8)
    check_rows(m, ref, "select + att + counts")
    m.close()
    assert_within(got, ref, layouts, "select + att + counts")


def test_with_backward_ext():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    m = make_model(sh, params, masks)
    put(m, batch, candidates=cand)
    got = ext_step(m, G, HOP_W)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = cand_ref.step(sh, params, batch, masks, cand, HOP_W, extra=linear_F(G))
    assert_within(got, ref, layouts, "rau_backward_ext")


def test_table_bank_device_and_question_batches_give_the_plain_batch_bits():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])
    image_of = np.array([0, 1, 2, 3, 4, 0, 1, 2], np.int32)
    table = np.ascontiguousarray(batch["feats"][:5])
    feats = np.ascontiguousarray(table[image_of])
    m = make_model(sh, params, masks)
    m.set_batch(feats, batch["tokens"], batch["lens"], batch["labels"], candidates=cand)
    want = dev_step(m, HOP_W)
    rows = m.loss_rows()
    m.set_batch(table, batch["tokens"], batch["lens"], batch["labels"], image_of=image_of, candidates=cand)
    assert m.batch_images() == 5 and m.batch_candidates == 5
    same_bits(dev_step(m, HOP_W), want)
    assert np.array_equal(m.loss_rows(), rows)
    m.bank_create(7)
    m.bank_put(1, table)
    m.set_batch(None, batch["tokens"], batch["lens"], batch["labels"], bank_rows=np.arange(1, 6, dtype=np.int32),
                image_of=image_of, candidates=cand)
    assert m.batch_candidates == 5
    same_bits(dev_step(m, HOP_W), want)
    x = torch.as_tensor(feats).cuda()
    torch.cuda.synchronize()
    m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"], candidates=cand)
    assert m.batch_candidates == 5
    same_bits(dev_step(m, HOP_W), want)
    # an attached question: set behind the upload or handed over with it; the list stays with the batch
    q = torch.as_tensor(np.random.default_rng(8).normal(size=(sh.B, 4 * sh.Rq)).astype(np.float32) * 0.5).cuda()
    torch.cuda.synchronize()
    m.set_batch(feats, batch["tokens"], batch["lens"], batch["labels"], candidates=cand)
    m.set_question(q)
    assert m.batch_question and m.batch_candidates == 5
    q_want = dev_step(m, HOP_W)
    assert any(not np.array_equal(q_want[k], want[k]) for k in GROUPS)
    m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"], question=q, candidates=cand)
    same_bits(dev_step(m, HOP_W), q_want)
    m.clear_candidates()
    assert m.batch_question
    q_plain = dev_step(m, HOP_W)
    assert any(not np.array_equal(q_plain[k], q_want[k]) for k in GROUPS)
    # every answer a candidate: the restricted criterion is the full-vocabulary one up to its summation order
    m.set_candidates(np.tile(np.arange(1, sh.K + 1, dtype=np.int32), (sh.B, 1)))
    layouts = {k: m.layout(k) for k in GROUPS}
    q_all = dev_step(m, HOP_W)
    m.close()
    # per layer slice on the scale of its parameter group: a slice whose true gradient is zero (attscore.bias: the
    # softmax is shift-invariant) holds rounding noise only, so its own magnitude is no scale
    for grp in GROUPS:
        scale = np.max(np.abs(q_plain[grp]))
        for name, sl in util.layer_slices(layouts[grp]):
            e = float(np.max(np.abs(q_all[grp][sl] - q_plain[grp][sl])) / (scale if scale > 0 else 1.0))
            assert e < 1e-5, (name, e)
    del x, q


def test_module_level_feval_routes_to_the_restricted_criterion():
    sh, batch, params, masks = problem("SMALL")
    cand = candidates(sh, batch["labels"])
    m = make_model(sh, params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.zero_grads()
    losses, _ans = modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32),
                                 cuda(batch["lens"], torch.int32), cuda(batch["labels"], torch.int32), HOP_W,
                                 candidates=cuda(cand, torch.int32))
    m.sync()
    g_mod = m.get_grads()
    put(m, batch, candidates=cand)
    g_step = dev_step(m, HOP_W)
    step_losses = m.losses()
    m.close()
    assert util.rel_err(losses.numpy(), step_losses) < 1e-5
    ref = cand_ref.step(sh, params, batch, masks, cand, HOP_W)
    assert_within(g_mod, ref, layouts, "feval(candidates=) vs the oracle")
    assert_within(g_step, ref, layouts, "step path vs the oracle")
