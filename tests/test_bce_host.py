"""The sigmoid answer head (rau_set_answer_loss, RAU_LOSS_BCE) on the host side: the places that declare the switch and
the two module-level calls (include/rau.h, bindings/rau.lua, rau_vqa_amd/_lib.py), predict.py's numpy statement of the
criterion -- bce_target bit for bit, soft_bce / soft_bce_grad in float32 against torch fp64 and against each other --
and tests/bce_ref.py against tests/merge_ref.py where the two must agree.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from rau_vqa_amd import _lib, predict
from tests import bce_ref, merge_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = (
    "int rau_set_answer_loss(rau_ctx* ctx, int kind);",
    "int rau_answer_loss(rau_ctx* ctx, int* kind);",
    "int rau_criterion_forward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, "
    "int32_t G, const int32_t* ids_dev, const float* w_dev, float* loss);",
    "int rau_criterion_backward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, "
    "int32_t G, const int32_t* ids_dev, const float* w_dev, float scale, float** d_logits);",
)
EXTREME = np.array([-1e4, -90, -20, 0, 20, 90, 1e4], np.float32)


def _code(text):
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))


def test_header_declares_the_switch_and_the_module_calls_and_keeps_the_abi_version():
    header = _code(open(os.path.join(ROOT, "include", "rau.h")).read())
    for p in PROTOS:
        assert p in header, p
    assert "#define RAU_LOSS_CE 0 " in header and "#define RAU_LOSS_BCE 1 " in header
    assert "#define RAU_ABI_VERSION 5 " in header
    assert (_lib.LOSS_CE, _lib.LOSS_BCE) == (0, 1) and _lib.LOSSES == {"ce": 0, "bce": 1}


def test_lua_shim_declares_and_wraps_them():
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    cdef = _code("\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S)))
    for p in PROTOS:
        assert p in cdef, p
    assert "function RAU:setAnswerLoss(kind)" in lua and "function RAU:answerLoss()" in lua
    for name in ("rau_set_answer_loss", "rau_answer_loss", "rau_criterion_forward_bce", "rau_criterion_backward_bce"):
        assert "C.%s(" % name in lua, name


def test_ctypes_table_binds_the_four_calls():
    assert _lib._SIGS["rau_set_answer_loss"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib._SIGS["rau_answer_loss"][1][1] is C.POINTER(C.c_int)
    assert len(_lib._SIGS["rau_criterion_forward_bce"][1]) == 8
    assert len(_lib._SIGS["rau_criterion_backward_bce"][1]) == 9
    bound = _lib.lib()
    # argument checks that need no device
    assert bound.rau_set_answer_loss(None, 1) == -1 and b"null" in bound.rau_last_error()
    assert bound.rau_answer_loss(None, None) == -1


# ---------------------------------------------------------------- bce_target
def test_bce_target_duplicates_empty_entries_rows_without_entries_and_the_end_ids():
    K = 7
    ids = np.array([[3, 3, 0, 5],      # a duplicate whose weights sum above 1; an empty entry that carries a weight
                    [0, 0, 0, 0],      # a row without entries
                    [1, K, 0, 0],      # ids 1 and K
                    [2, 2, 2, 0]],     # a duplicate below 1: added in entry order in float32
                   np.int32)
    w = np.array([[0.75, 0.5, 0.9, 0.25],
                  [0.5, 0.5, 0.5, 0.5],
                  [1.0, 0.125, 0.7, 0.7],
                  [0.1, 0.2, 0.3, 0.9]], np.float32)
    t = predict.bce_target(ids, w, K)
    assert t.dtype == np.float32 and t.shape == (4, K)
    want = np.zeros((4, K), np.float32)
    want[0, 2], want[0, 4] = 1.0, 0.25
    want[2, 0], want[2, K - 1] = 1.0, 0.125
    want[3, 1] = (np.float32(0) + np.float32(0.1) + np.float32(0.2)) + np.float32(0.3)
    assert np.array_equal(t.view(np.uint32), want.view(np.uint32))
    assert t[0, 2] == np.float32(1)                               # clamped to exactly 1
    assert not t[1].any()
    # ids outside [0, K] are clamped as the device clamps them: below 0 is empty, above K is K
    t2 = predict.bce_target(np.array([[-3, K + 9]], np.int32), np.array([[0.5, 0.25]], np.float32), K)
    assert t2[0, K - 1] == np.float32(0.25) and t2.sum() == np.float32(0.25)
    # labels are the one-entry sets of weight 1
    y = np.array([1, K, 4], np.int32)
    assert np.array_equal(predict.bce_target_labels(y, K), np.eye(K, dtype=np.float32)[y - 1])


# ---------------------------------------------------------------- soft_bce / soft_bce_grad
def problem(B, K, G, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, K)) * 3).astype(np.float32)
    x[0, :EXTREME.size] = EXTREME
    x[1, :EXTREME.size] = EXTREME[::-1]
    ids = rng.integers(0, K + 1, (B, G)).astype(np.int32)
    ids[0, :3] = (1, 4, 7)                                       # targets on the extreme logits of row 0
    ids[1, :2] = 3                                               # a duplicate pair summing above 1
    ids[2] = 0                                                   # an unlabelled row
    w = (rng.integers(0, 9, (B, G)) / 8).astype(np.float32)
    w[1, :2] = 0.75
    w[3] = 0                                                     # labelled, with the all-zero target
    ids[3, 0] = 2
    return x, ids, w


def torch_bce(x, ids, w):
    """(rows [B], mean, gradient of the mean) in fp64: binary_cross_entropy_with_logits, unlabelled rows zeroed"""
    B, K = x.shape
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(predict.bce_target(ids, w, K), dtype=torch.float64)
    live = torch.tensor((ids > 0).any(axis=1).astype(np.float64))
    rows = torch.nn.functional.binary_cross_entropy_with_logits(xt, t, reduction="none").sum(1) * live
    mean = rows.sum() / B
    mean.backward()
    return rows.detach().numpy(), float(mean.detach()), xt.grad.numpy()


@pytest.mark.parametrize("B,K,G", [(6, 12, 4), (5, 1000, 10), (4, 257, 3)])
def test_float32_statement_against_torch_fp64(B, K, G):
    x, ids, w = problem(B, K, G, seed=K)
    rows, mean = predict.soft_bce(x, ids, w)
    g = predict.soft_bce_grad(x, ids, w)
    assert rows.dtype == np.float32 and g.dtype == np.float32 and isinstance(mean, np.float32)
    assert np.isfinite(rows).all() and np.isfinite(g).all() and np.isfinite(mean)
    ref_rows, ref_mean, ref_g = torch_bce(x, ids, w)
    err = {"rows": util.rel_err(rows, ref_rows), "mean": abs(float(mean) - ref_mean) / abs(ref_mean),
           "grad": util.rel_err(g, ref_g)}
    print(err)
    assert all(v <= 1e-6 for v in err.values()), err
    assert rows[2] == 0 and not g[2].any() and not np.signbit(g[2]).any()      # the unlabelled row: 0 and +0
    assert rows[3] > 0 and (g[3] > 0).all()                                    # the all-zero target pushes down


def test_gradient_equals_a_central_difference_of_the_loss_in_fp64():
    B, K, G = 4, 9, 3
    x, ids, w = problem(B, K, G, seed=5)
    x = np.clip(x.astype(np.float64), -30, 30)                   # differences of the extreme entries are all rounding
    g = predict.soft_bce_grad(x, ids, w, dtype=np.float64)
    assert g.dtype == np.float64
    h = 1e-5
    fd = np.zeros_like(x)
    for b in range(B):
        for k in range(K):
            d = np.zeros_like(x)
            d[b, k] = h
            fd[b, k] = (predict.soft_bce(x + d, ids, w, dtype=np.float64)[1]
                        - predict.soft_bce(x - d, ids, w, dtype=np.float64)[1]) / (2 * h)
    assert np.max(np.abs(g - fd)) < 1e-8 * max(1.0, np.max(np.abs(g)))


def test_set_stats_takes_the_loss_kind():
    rng = np.random.default_rng(3)
    H, B, K, G = 3, 9, 12, 4
    lg = rng.standard_normal((H, B, K)).astype(np.float32)
    dp = rng.uniform(size=(H, B)).astype(np.float32)
    _x, ids, w = problem(B, K, G, seed=2)
    ce, bce = predict.set_stats(lg, dp, ids, w), predict.set_stats(lg, dp, ids, w, loss="bce")
    for k in ce:
        if k != "loss":
            assert np.array_equal(ce[k], bce[k]), k
    for h in range(H):
        assert bce["loss"][h] == predict.soft_bce(lg[h], ids, w)[1]
    assert np.array_equal(ce["loss"], predict.set_stats(lg, dp, ids, w, loss="ce")["loss"])
    with pytest.raises(ValueError):
        predict.set_stats(lg, dp, ids, w, loss="hinge")


# ---------------------------------------------------------------- bce_ref
def test_reference_forward_does_not_depend_on_the_loss():
    sh = util.shapes(util.SMALL)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    ce = merge_ref.step(sh, params, batch, masks, hop_w, backward=False)
    # one-hot targets through the set form: the labels as one entry of weight 1
    ids = np.asarray(batch["labels"], np.int32)[:, None]
    bce = bce_ref.step(sh, params, batch, masks, hop_w, answers=(ids, np.ones_like(ids, np.float32)))
    assert np.array_equal(bce["logits"], ce["logits"]) and np.array_equal(bce["dopred"], ce["dopred"])
    lab = bce_ref.step(sh, params, batch, masks, hop_w)
    assert np.array_equal(lab["losses"], bce["losses"])
    for g in bce_ref.GROUPS:
        assert np.array_equal(lab["g_" + g], bce["g_" + g]), g
    # and its losses are the numpy statement's
    for h in range(sh.H):
        want = predict.soft_bce(bce["logits"][h], ids, np.ones_like(ids, np.float32), dtype=np.float64)[1]
        assert abs(bce["losses"][h] - want) <= 1e-12 * abs(want)
