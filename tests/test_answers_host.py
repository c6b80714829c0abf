"""Answer sets (rau_set_answers) on the host side: the header, the Lua cdef and the ctypes table declare the new
entry points alike; predict.py's numpy statement of the contract (soft_ce, answer_score, set_correct) behaves as
include/rau.h says; loader.vqa_scores; loader.feed / SlotFeeder attach a set only when the QuestionSet has one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rau_vqa_amd import _lib, joint, loader, predict, t7
from rau_vqa_amd.model import RAU, Config
from tests.test_abi import ROOT, _normalise, _prototypes

WANT = {
    "rau_set_answers": "int rau_set_answers(rau_ctx* ctx, int slot, int32_t G, const int32_t* ids, const float* w, "
                       "const float* score)",
    "rau_batch_answers": "int rau_batch_answers(rau_ctx* ctx, int32_t* G)",
    "rau_step_scores": "int rau_step_scores(rau_ctx* ctx, float* per_sample, float* total)",
    "rau_predict_scores": "int rau_predict_scores(rau_ctx* ctx, float* oe, float* mc, float* totals)",
    "rau_criterion_forward_set": "int rau_criterion_forward_set(rau_ctx* ctx, int h, const float* logits, int32_t G, "
                                 "const int32_t* ids_dev, const float* w_dev, float* loss)",
    "rau_criterion_backward_set": "int rau_criterion_backward_set(rau_ctx* ctx, int h, const float* logits, "
                                  "int32_t G, const int32_t* ids_dev, const float* w_dev, float scale, "
                                  "float** d_logits)",
}
DIMS = dict(B=8, T=5, V=30, E=8, Rq=4, D=4, S=4, M=8, A=4, R=4, K=10, H=2)


def test_header_has_the_prototypes_and_keeps_the_abi_version():
    header = open(os.path.join(ROOT, "include", "rau.h")).read()
    got = _prototypes(header)
    for name, proto in WANT.items():
        assert got.get(name) == _normalise(proto), name
    assert "#define RAU_ABI_VERSION 5" in header            # additive, like every call since version 5
    assert "#define RAU_MAX_ANSWERS 16" in header


def test_ctypes_table_has_the_header_arities():
    header = _prototypes(open(os.path.join(ROOT, "include", "rau.h")).read())
    for name in WANT:
        res, args = _lib._SIGS[name]
        params = header[name][header[name].index("(") + 1:-1].split(", ")
        assert res is C.c_int and len(args) == len(params), name
    assert _lib._SIGS["rau_set_answers"][1][1:3] == [C.c_int, C.c_int32]
    assert _lib._SIGS["rau_criterion_backward_set"][1][6] is C.c_float


def test_lua_cdef_and_wrappers_agree_with_the_header():
    header = _prototypes(open(os.path.join(ROOT, "include", "rau.h")).read())
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    cdef = _prototypes("\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S)))
    for name in WANT:
        assert cdef.get(name) == header[name], name
    for fn in ("RAU:setAnswers", "RAU:batchAnswers", "RAU:stepScores", "RAU:predictScores",
               "RAU:criterionForwardSet", "RAU:criterionBackwardSet"):
        assert re.search(r"function\s+" + re.escape(fn) + r"\b", lua), fn


def test_library_exports_the_entry_points_and_rejects_a_null_context():
    l = _lib.lib()
    assert l.rau_set_answers(None, -1, 1, None, None, None) == -1
    assert l.rau_batch_answers(None, None) == -1
    assert l.rau_step_scores(None, None, None) == -1
    assert l.rau_predict_scores(None, None, None, None) == -1
    assert l.rau_criterion_forward_set(None, 0, None, 1, None, None, None) == -1
    assert l.rau_criterion_backward_set(None, 0, None, 1, None, None, 1.0, None) == -1


# ---- the numpy statement of the contract
def _rows(seed=0, B=9, K=11):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, K)) * 3).astype(np.float32), rng


def test_soft_ce_is_the_single_label_criterion_for_one_unit_entry():
    pred, rng = _rows()
    y = rng.integers(1, pred.shape[1] + 1, pred.shape[0])
    rows, mean = predict.soft_ce(pred, y[:, None], np.ones((len(y), 1), np.float32))
    assert mean == joint.cross_entropy(pred, y)                       # bit for bit
    # fifteen empty entries behind the label change nothing, whatever their weights
    ids = np.zeros((len(y), 16), np.int64)
    ids[:, 0] = y
    w = rng.random((len(y), 16)).astype(np.float32)
    w[:, 0] = 1
    rows16, mean16 = predict.soft_ce(pred, ids, w)
    assert np.array_equal(rows16, rows) and mean16 == mean


def test_soft_ce_is_linear_in_the_weights():
    pred, rng = _rows(1)
    B, K = pred.shape
    ids = rng.integers(0, K + 1, (B, 3))
    ids[0] = 0                                                        # a row without entries
    ids[1] = [4, 4, 2]                                                # a duplicate adds up
    w1, w2 = rng.random((B, 3)).astype(np.float32), rng.random((B, 3)).astype(np.float32)
    r1, r2 = predict.soft_ce(pred, ids, w1)[0], predict.soft_ce(pred, ids, w2)[0]
    r12 = predict.soft_ce(pred, ids, 2 * w1 + w2)[0]
    np.testing.assert_allclose(r12, 2 * r1.astype(np.float64) + r2, rtol=2e-6, atol=1e-6)
    assert r1[0] == 0 and r12[0] == 0
    single = predict.soft_ce(pred[1:2], np.array([[4]]), np.array([[w1[1, 0] + w1[1, 1]]], np.float32))[0][0]
    two = predict.soft_ce(pred[1:2], np.array([[4, 4]]), w1[1:2, :2])[0][0]
    assert two == pytest.approx(single, rel=1e-6)
    # the gradient statement: rows sum to zero (softmax mass W/B against W/B of one-hots), zero on the empty row
    g = predict.soft_ce_grad(pred, ids, w1)
    np.testing.assert_allclose(g.sum(1), 0, atol=1e-12)
    assert not g[0].any()
    eps = 1e-6
    mean32 = predict.soft_ce(pred, ids, w1)[1]                        # the float32 statement; differences in f64
    p64 = pred.astype(np.float64)

    def f(p):
        lse = np.log(np.exp(p - p.max(1, keepdims=True)).sum(1)) + p.max(1)
        wz = np.where(ids > 0, w1, 0).astype(np.float64)
        return sum(wz[b, j] * (lse[b] - p[b, ids[b, j] - 1]) for b in range(B) for j in range(3) if ids[b, j] > 0) / B
    d = np.zeros_like(p64)
    d[2, 5] = eps
    assert (f(p64 + d) - f(p64 - d)) / (2 * eps) == pytest.approx(g[2, 5], abs=1e-7)
    assert mean32 == pytest.approx(f(p64), rel=1e-5)


def test_answer_score_and_the_correct_rule():
    ids = np.array([[3, 0, 3, 5], [0, 0, 0, 0], [2, 7, 0, 1], [4, 4, 4, 4]])
    sc = np.array([[0.3, 9.0, 0.6, 1.0], [1, 1, 1, 1], [0.0, 1.0, 5.0, 0.9], [0.1, 0.2, 0.3, 0.4]], np.float32)
    ans = np.array([[3, 1, 2, 4], [5, 3, 7, 1], [1, 1, 1, 5]])
    got = predict.answer_score(ans, ids, sc)
    f = np.float32
    want = np.array([[f(0.3) + f(0.6), 0, 0, ((f(0.1) + f(0.2)) + f(0.3)) + f(0.4)],
                     [1.0, 0, 1.0, 0],
                     [0, 0, 0.9, 0]], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)      # duplicates add in entry order, 0 never matches
    ok = predict.set_correct(ans, ids, sc)
    assert np.array_equal(ok, want > 0)
    assert not predict.set_correct(np.array([2]), ids[2:3], sc[2:3])[0]   # in the set, but with score 0
    assert not predict.set_correct(np.arange(1, 9)[:, None], ids[1:2], sc[1:2]).any()   # a row without entries


def test_set_stats_reduces_to_feval_stats_for_one_unit_entry():
    rng = np.random.default_rng(5)
    H, B, K = 3, 13, 7
    logits = rng.standard_normal((H, B, K)).astype(np.float32)
    dopred = rng.random((H, B)).astype(np.float32)
    y = rng.integers(1, K + 1, B)
    a = predict.set_stats(logits, dopred, y[:, None], np.ones((B, 1), np.float32))
    b = joint.feval_stats(logits, dopred, y)
    for k in ("loss", "loss_do_pred", "correct", "do_pred_correct", "fired", "selected"):
        assert np.array_equal(a[k], b[k]), k
    assert a["did_correct"] == b["did_correct"]
    assert np.array_equal(a["ans"][H], b["uni_ans"]) and np.array_equal(a["ans"][H + 1], b["select_ans"])


def test_vqa_scores():
    got = loader.vqa_scores(np.array([[0, 1, 2, 3, 4, 10]]))
    assert got.dtype == np.float32 and got.shape == (1, 6)
    assert np.array_equal(got, np.array([[0, np.float32(1) / np.float32(3), np.float32(2) / np.float32(3), 1, 1, 1]],
                                        np.float32))


# ---- the driver: shapes are checked before the library is called
class _RecLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name,) + args[1:])
            return 0
        return fn


def _rau():
    m = RAU.__new__(RAU)
    m.cfg = Config(**DIMS)
    m._lib, m._h, m._n = _RecLib(), None, m.cfg.B
    return m


def test_driver_checks_the_set_and_passes_slot_and_G():
    m = _rau()
    ids, w = np.ones((8, 3), np.int32), np.ones((8, 3), np.float32)
    for bad in ((ids[:5], w[:5]), (ids, w[:, :2]), (np.ones((8, 17), np.int32), np.ones((8, 17), np.float32)),
                (ids, w, w[:, :1])):
        with pytest.raises(ValueError):
            m.set_answers(*bad)
    assert m._lib.calls == []
    m.set_answers(ids, w)
    m.set_answers(ids, w, w, slot=1)
    (n0, s0, g0, *p0), (n1, s1, g1, *p1) = m._lib.calls
    assert (n0, s0, g0, p0[2]) == ("rau_set_answers", -1, 3, None) and (n1, s1, g1) == ("rau_set_answers", 1, 3)
    assert p1[2] is not None
    # set_batch(..., answers=) is set_answers after the upload; without it nothing new is called
    rng = np.random.default_rng(0)
    batch = dict(feats=rng.standard_normal((8, 4, 4)).astype(np.float32), tokens=np.ones((5, 8), np.int32),
                 lens=np.full(8, 3, np.int32), labels=np.ones(8, np.int32))
    m._lib.calls.clear()
    m.set_batch(**batch)
    m.set_batch_async(0, **batch)
    assert [c[0] for c in m._lib.calls] == ["rau_set_batch_typed", "rau_set_batch_async_typed"]
    m._lib.calls.clear()
    m.set_batch(**batch, answers=(ids, w))
    m.set_batch_async(1, **batch, answers=(ids, w, w))
    assert [c[0] for c in m._lib.calls] == ["rau_set_batch_typed", "rau_set_answers", "rau_set_batch_async_typed",
                                            "rau_set_answers"]
    assert m._lib.calls[1][1] == -1 and m._lib.calls[3][1] == 1
    assert m.step_scores()[0].shape == (4, 8) and m.predict_scores(mc=True)[1].shape == (4, 8)


# ---- loader: answer sets travel with the batch only when the QuestionSet has them
N, T, D, W, H, NIMG, TB, G = 12, 5, 4, 2, 2, 4, 3, 4


@pytest.fixture()
def split(tmp_path):
    rng = np.random.default_rng(3)
    names = [f"train2014/COCO_train2014_{i:012d}.jpg" for i in range(NIMG)]
    fdir = tmp_path / "feat"
    fdir.mkdir()
    for name in names:
        t7.save(fdir / loader.feature_name(name), rng.standard_normal((D, W, H)).astype(np.float32))
    lens = rng.integers(1, T + 1, N)
    q = np.zeros((N, T), np.int32)
    for i, l in enumerate(lens):
        q[i, :l] = rng.integers(2, 9, l)
    base = dict(question=q, lengths_q=lens, img_list=rng.integers(1, NIMG + 1, N), question_id=np.arange(N),
                answers=rng.integers(1, 11, N))
    counts = rng.integers(0, 5, (N, G))
    sets = dict(ans_ids=rng.integers(0, 11, (N, G)), ans_w=(counts / 10).astype(np.float32),
                ans_score=loader.vqa_scores(counts))

    def make(with_sets, score=True):
        kw = dict(base, **sets) if with_sets else dict(base)
        if with_sets and not score:
            kw["ans_score"] = None
        return loader.DataClass(loader.QuestionSet(**kw), names, TB, "train")
    return make, str(fdir), sets


class _FakeRau:
    """The calls feed and SlotFeeder make; records them."""

    def __init__(self):
        self.capacity = self.batch_size = TB
        self.calls = []
        self.stage = [{"feats": np.zeros((TB, D, W * H), np.float32), "tokens": np.zeros((T, TB), np.int32),
                       "lens": np.zeros(TB, np.int32), "labels": np.zeros(TB, np.int32)} for _ in range(2)]

    def set_batch(self, feats, tokens, lens, labels=None, **kw):
        self.calls.append(("set_batch", labels))

    def batch_slot(self, slot, feat_type="f32"):
        return self.stage[slot]

    def set_batch_async(self, slot, has_labels=True, **kw):
        self.calls.append(("set_batch_async", slot))

    def set_answers(self, ids, w, score=None, slot=None):
        self.calls.append(("set_answers", slot, ids, w, score))

    def use_batch(self, slot):
        self.calls.append(("use_batch", slot))


def test_next_batch_feat_keeps_its_tuple(split):
    make, fdir, sets = split
    plain, withs = make(False), make(True)
    a, b = plain.next_batch_feat(fdir, D, W, H), withs.next_batch_feat(fdir, D, W, H)
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert plain.last_answers is None
    ids, w, sc = withs.last_answers
    idx = np.arange(TB)                                           # batch order 2: in order
    assert ids.dtype == np.int32 and w.dtype == np.float32 and sc.dtype == np.float32
    np.testing.assert_array_equal(ids, sets["ans_ids"][idx])
    np.testing.assert_array_equal(w, sets["ans_w"][idx])
    np.testing.assert_array_equal(sc, sets["ans_score"][idx])
    assert len(make(True, score=False).next_batch_feat(fdir, D, W, H)) == 5
    assert len(withs.next_batch_feat(fdir, D, W, H, unique=True)) == 6


def test_feed_attaches_a_set_only_when_there_is_one(split):
    make, fdir, sets = split
    d, rau = make(False), _FakeRau()
    loader.feed(rau, d.next_batch_feat(fdir, D, W, H), answers=d.last_answers)
    loader.feed(rau, d.next_batch_feat(fdir, D, W, H))
    assert [c[0] for c in rau.calls] == ["set_batch", "set_batch"]
    d, rau = make(True, score=False), _FakeRau()
    loader.feed(rau, d.next_batch_feat(fdir, D, W, H), answers=d.last_answers)
    assert [c[0] for c in rau.calls] == ["set_batch", "set_answers"]
    _, slot, ids, w, score = rau.calls[1]
    assert slot is None and score is None and ids.shape == w.shape == (TB, G)
    np.testing.assert_array_equal(ids, sets["ans_ids"][:TB])


def test_slot_feeder_attaches_a_set_only_when_there_is_one(split):
    make, fdir, sets = split
    rau = _FakeRau()
    feeder = loader.SlotFeeder(rau, make(False), fdir, D, W, H)
    feeder.next()
    assert [c[0] for c in rau.calls] == ["set_batch_async", "use_batch"] * 2
    rau = _FakeRau()
    feeder = loader.SlotFeeder(rau, make(True), fdir, D, W, H)
    feeder.next()
    assert [c[0] for c in rau.calls] == ["set_batch_async", "set_answers", "use_batch"] * 2
    for k, first in ((1, 0), (4, TB)):                            # behind the upload, into the same slot
        _, slot, ids, w, score = rau.calls[k]
        assert slot == rau.calls[k - 1][1] == rau.calls[k + 1][1]
        np.testing.assert_array_equal(ids, sets["ans_ids"][first:first + TB])
        np.testing.assert_array_equal(score, sets["ans_score"][first:first + TB])
