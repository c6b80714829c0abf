"""predict.top_answers: the numpy statement of the ranked-answer contract of rau_dev_topk / rau_topk
(include/rau.h), which the GPU tests then trust; and the three places that declare the two symbols."""
import os
import re

import numpy as np
import pytest

from rau_vqa_amd import predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def rows(*r):
    return np.array([r], np.float32)[None]       # [1, 1, K]


def test_ties_resolve_to_the_lower_index_at_every_rank():
    ids, score, _ = predict.top_answers(rows(2, 5, 2, 5, 5, 1, 2), 7)
    assert ids[0, 0].tolist() == [2, 4, 5, 1, 3, 7, 6]
    assert score[0, 0].tolist() == [5, 5, 5, 2, 2, 2, 1]
    ids, _, _ = predict.top_answers(np.zeros((2, 3, 9), np.float32), 4)      # all equal
    assert np.array_equal(ids, np.broadcast_to(np.arange(1, 5, dtype=np.int32), (2, 3, 4)))


def test_positive_and_negative_zero_tie_and_keep_their_sign():
    x = rows(-0.0, 0.0, -1, 0.0, -0.0)
    ids, score, _ = predict.top_answers(x, 5)
    assert ids[0, 0].tolist() == [1, 2, 4, 5, 3]
    assert np.array_equal(score.view(np.uint32), x[..., [0, 1, 3, 4, 2]].view(np.uint32))
    assert np.signbit(score[0, 0]).tolist() == [True, False, False, True, True]


def test_infinities_order_as_values_and_nan_comes_last_by_index():
    x = rows(NAN, -INF, 3, NAN, INF, -2, NAN)
    ids, score, _ = predict.top_answers(x, 7)
    assert ids[0, 0].tolist() == [5, 3, 6, 2, 1, 4, 7]
    assert np.isnan(score[0, 0, 4:]).all() and score[0, 0, 3] == -INF
    # payloads and signs of NaN survive: the scores are the entries themselves
    y = np.array([0x7fc00001, 0xffc00002, 0x7f800003], np.uint32).view(np.float32)[None, None]
    ids, score, _ = predict.top_answers(y, 3)
    assert ids[0, 0].tolist() == [1, 2, 3]
    assert np.array_equal(score.view(np.uint32), y.view(np.uint32))
    ids, _, _ = predict.top_answers(np.full((1, 2, 6), NAN, np.float32), 6)   # all NaN
    assert np.array_equal(ids[0], np.broadcast_to(np.arange(1, 7, dtype=np.int32), (2, 6)))


def test_full_ranking_is_a_permutation_in_descending_order():
    rng = np.random.default_rng(0)
    x = rng.integers(-3, 4, size=(4, 6, 17)).astype(np.float32)              # many ties
    x[0, 0, 3], x[1, 2, 5], x[2, 1, 0] = NAN, INF, -INF
    ids, score, _ = predict.top_answers(x, 17)
    assert np.array_equal(np.sort(ids, -1), np.broadcast_to(np.arange(1, 18, dtype=np.int32), ids.shape))
    assert np.array_equal(score.view(np.uint32), np.take_along_axis(x, ids - 1, -1).view(np.uint32))
    a, b = score[..., :-1], score[..., 1:]
    assert np.all((a > b) | ((a == b) & (ids[..., :-1] < ids[..., 1:])) | np.isnan(b))
    for k in (1, 5):                                                         # a prefix of the full ranking
        assert np.array_equal(predict.top_answers(x, k)[0], ids[..., :k])
    for k in (0, 18):
        with pytest.raises(ValueError):
            predict.top_answers(x, k)


def test_rank_0_is_first_max_and_accepts_merge_hops_lists():
    rng = np.random.default_rng(1)
    tab = [rng.integers(-2, 3, size=(9, 11)).astype(np.float32) for _ in range(5)]
    ids, score, _ = predict.top_answers(tab, 3)
    assert ids.shape == (5, 9, 3) and ids.dtype == np.int32 and score.dtype == np.float32
    for r, p in enumerate(tab):
        assert np.array_equal(ids[r, :, 0], predict.first_max(p))
        assert np.array_equal(score[r, :, 0], p.max(1))


def test_confidences_are_the_softmax_and_a_full_ranking_sums_to_one():
    rng = np.random.default_rng(2)
    x = (4 * rng.standard_normal((3, 7, 1000))).astype(np.float32)
    ids, score, conf = predict.top_answers(x, 1000)
    assert conf.dtype == np.float32
    assert np.all(np.abs(conf.astype(np.float64).sum(-1) - 1.0) < 1e-6)
    e = np.exp(x.astype(np.float64) - x.max(-1, keepdims=True))
    soft = e / e.sum(-1, keepdims=True)
    assert np.array_equal(conf, np.take_along_axis(soft, ids - 1, -1).astype(np.float32))
    assert np.all(conf[..., :-1] >= conf[..., 1:])
    assert np.array_equal(predict.top_answers(x, 5)[2], conf[..., :5])


def test_header_lua_cdef_and_ctypes_table_declare_both_symbols():
    from rau_vqa_amd import _lib
    header = open(os.path.join(ROOT, "include", "rau.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    for sym in ("rau_dev_topk", "rau_topk"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, cdef), sym
        assert sym in _lib._SIGS
    assert len(_lib._SIGS["rau_dev_topk"][1]) == 7 and len(_lib._SIGS["rau_topk"][1]) == 5
    assert re.search(r"function\s+RAU:topk\b", lua) and re.search(r"function\s+Tensor:topk\b", lua)
