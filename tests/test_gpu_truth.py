"""Which ground truth is in force (csrc: Truth, truth_of, MergeState::truth): what the other files leave open.

Every comparison is raw-bit equality between two routes to the same numbers on one context; nothing is compared
against a host restatement with a tolerance, and no case provokes a refusal.

a. the target of the last forward outlives a slot switch: rau_step_stats and rau_step_scores read the record the
   forward left, not the resident batch.  The backward leg cannot follow the switch directly: rau_use_batch ends
   the open forward pass (include/rau.h: every state rule of rau_backward applies), so rau_backward_select there is
   RAU_ERR_STATE before and after this file existed.  What is asserted instead is the round trip: back on slot 0,
   the same forward and rau_backward_select give the gradients of the run that never left the slot.
b. a captured step reads the resident batch's target on every replay (not the one it was captured with).
c. the module-level criterion with labels_dev = NULL reads the resident batch's target, set or labels.  A slot's
   own device pointers are not reachable through the ABI: the explicit calls get device copies of the same values.
d. rau_topk's staging is regrown (the one region freed before rau_destroy) and set_batch_size then clears every
   scratch region: the freed one must be gone from that list."""
import ctypes as C

import numpy as np
import pytest

from rau_vqa_amd import _lib as L
from rau_vqa_amd import predict
from tests import util
from tests.test_gpu_answers import STAT_KEYS, answer_set, make

pytestmark = pytest.mark.gpu

PADS = dict(B=6, T=5, V=50, E=8, Rq=16, D=24, S=49, M=40, A=20, R=16, K=40, H=3)   # Sp = 52: pad columns in play


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_grads(a, b):
    return all(same(a[g], b[g]) for g in ("embed", "rnn", "mult"))


def queries(m):
    s = m.step_stats()
    per, tot = m.step_scores()
    return [np.asarray(s[k]) for k in STAT_KEYS] + [np.int32([s["did_correct"]]), per, tot]


# ---------------------------------------------------------------- a
def test_forward_target_outlives_a_slot_switch():
    m, sh, batch, _, masks = make(util.SMALL)
    other, _, _ = util.make_problem(sh, seed=77, scale=0.5)
    ids, w, score = answer_set(util.SMALL, 3, seed=2)
    assert len(np.unique(w)) > 1
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    select_w = np.array([0.5, 1.0, 0.25], np.float32)[:sh.H]
    m.training()
    m.set_masks(masks)
    m.set_batch_async(0, batch["feats"], batch["tokens"], batch["lens"], None, has_labels=False,
                      answers=(ids, w, score))
    m.set_batch_async(1, other["feats"], other["tokens"], other["lens"], other["labels"])

    def run(switch):
        m.use_batch(0)
        m.zero_grads()
        m.forward()
        if switch:
            m.use_batch(1)                 # slot 0 is not uploaded into: its forward's record stays readable
            assert m.batch_answers == 0    # the resident batch has labels, the record an answer set
        q = queries(m)
        if switch:                         # the backward belongs to an open forward pass of the resident batch
            m.use_batch(0)
            m.zero_grads()
            m.forward()
        m.backward(hop_w, select_w)
        return q, m.get_grads()

    ref_q, ref_g = run(False)
    got_q, got_g = run(True)
    for k, a, b in zip(STAT_KEYS + ("did_correct", "per_sample", "total"), ref_q, got_q):
        assert same(a, b), k
    assert same_grads(ref_g, got_g)
    again_q, again_g = run(False)          # and the reference repeats itself
    assert all(same(a, b) for a, b in zip(ref_q, again_q)) and same_grads(ref_g, again_g)
    m.close()


# ---------------------------------------------------------------- b
def test_captured_step_reads_the_resident_target():
    m, sh, batch, _, masks = make(util.SMALL)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    select_w = np.array([0.5, 1.0, 0.25], np.float32)[:sh.H]
    first = answer_set(util.SMALL, 3, seed=5)
    second = answer_set(util.SMALL, 3, seed=6)
    assert not np.array_equal(first[0], second[0])
    m.training()
    m.set_masks(masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], None, answers=first)
    m.graph_step(hop_w, zero_grads=True, select_w=select_w)       # captured against the first set
    g_first = m.get_grads()
    m.set_answers(*second)                                        # same G: the same graph is replayed
    m.graph_step(hop_w, zero_grads=True, select_w=select_w)
    g_replay = m.get_grads()
    m.zero_grads()
    m.forward()
    m.backward(hop_w, select_w)
    g_eager = m.get_grads()
    assert same_grads(g_replay, g_eager)
    assert not same(g_first["mult"], g_replay["mult"])             # the two sets do give different gradients
    m.close()


# ---------------------------------------------------------------- c
def test_criterion_without_labels_argument_reads_the_resident_target():
    m, sh, batch, _, _ = make(util.SMALL)
    H, B, K = sh.H, sh.B, sh.K
    lib, h = m._lib, m._h
    ids, w, _ = answer_set(util.SMALL, 3, seed=8)
    logits = np.random.default_rng(4).standard_normal((B, K)).astype(np.float32)

    def dev(a):
        p = C.c_void_p()
        L.check(lib.rau_dev_alloc(h, a.size, C.byref(p)))
        L.check(lib.rau_dev_upload(h, p, a.ctypes.data, a.nbytes))
        return p

    def forward(fn, *target):
        loss = C.c_float()
        L.check(fn(h, 1, lg_d, *target, C.byref(loss)))
        return np.float32(loss.value)

    def backward(fn, scale, *target):
        q = C.c_void_p()
        L.check(fn(h, 1, lg_d, *target, scale, C.byref(q)))
        out = np.empty((B, K), np.float32)
        L.check(lib.rau_dev_download(h, out.ctypes.data, q, out.nbytes))
        return out
    lg_d, ids_d, w_d, y_d = dev(logits), dev(ids), dev(w), dev(batch["labels"].astype(np.int32))
    m.evaluate()
    # a batch with a set
    m.set_batch(**batch, answers=(ids, w))
    assert same(forward(lib.rau_criterion_forward, None), forward(lib.rau_criterion_forward_set, 3, ids_d, w_d))
    for scale in (1.0, float(H)):
        assert same(backward(lib.rau_criterion_backward, scale, None),
                    backward(lib.rau_criterion_backward_set, scale, 3, ids_d, w_d)), scale
    set_loss = forward(lib.rau_criterion_forward, None)
    # a labels-only batch
    m.set_batch(**batch)
    assert m.batch_answers == 0
    assert same(forward(lib.rau_criterion_forward, None), forward(lib.rau_criterion_forward, y_d))
    for scale in (1.0, float(H)):
        assert same(backward(lib.rau_criterion_backward, scale, None),
                    backward(lib.rau_criterion_backward, scale, y_d)), scale
    assert not same(set_loss, forward(lib.rau_criterion_forward, None))   # the two targets do differ
    m.close()


# ---------------------------------------------------------------- d
def test_topk_regrow_then_set_batch_size():
    m, sh, batch, _, _ = make(PADS)
    small, _, _ = util.make_problem(util.shapes(PADS, B=sh.B - 1), seed=5, scale=0.5)

    def check(k, tag):
        tab_pred, _ = predict.merge_hops(m.logits(), m.dopred(), m.attention())
        rid, rscore, _ = predict.top_answers(tab_pred, k)
        ids, score, _ = m.topk(k)
        assert ids.dtype == np.int32 and np.array_equal(ids, rid), tag
        assert score.dtype == np.float32 and same(score, np.ascontiguousarray(rscore, np.float32)), tag

    m.evaluate()
    m.set_batch(**batch)
    m.forward()
    check(2, "k2")
    check(5, "k5: the first staging buffer is freed")
    m.set_batch_size(sh.B - 1)             # clears every scratch region
    m.set_batch(**small)
    m.forward()
    check(5, "n-1")
    m.set_batch_size(sh.B)
    m.set_batch(**batch)
    m.forward()
    check(5, "back at n")
    check(7, "regrown after the resizes")
    m.close()
