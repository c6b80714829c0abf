"""Multiple-choice candidates on the host: the header and the bindings, the numpy statements of the restricted
criterion (predict.cand_ce / cand_bce and their gradients) against fp64 torch autograd, the ranked candidates
(predict.top_candidates) and the Python layer's argument checks.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from rau_vqa_amd import predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rau_set_candidates", "rau_batch_candidates", "rau_cand_stats", "rau_topk_cand",
         "rau_criterion_forward_cand", "rau_criterion_backward_cand")
TOL = 1e-6


# ------------------------------------------------------------------------------------------ header and bindings
def test_header_declares_the_calls_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "rau.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
    assert "#define RAU_ABI_VERSION 5" in code
    assert "#define RAU_MAX_CANDIDATES 32" in code


def test_library_and_bindings_carry_the_symbols():
    from rau_vqa_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    for name in CALLS:
        assert name in lua, name
    for fn in ("RAU:setCandidates", "RAU:candStats", "RAU:topkCand"):
        assert "function " + fn in lua, fn


# ------------------------------------------------------------------------------------------ numpy against torch
B, K, Cn, G = 9, 14, 6, 3


def case(kind, seed=0):
    """Logits, candidates, a truth and sample weights with every row class: 0 plain, 1 duplicates, 2 empties, 3 truth
    outside the list, 4 no live candidate, 5 a single candidate (its truth), 6 a duplicated truth entry, 7-8 plain."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, K)).astype(np.float32) * 2
    y = rng.integers(1, K + 1, size=B)
    cand = np.zeros((B, Cn), np.int64)
    for b in range(B):
        others = rng.permutation([k for k in range(1, K + 1) if k != y[b]])
        cand[b] = np.concatenate([[y[b]], others[:Cn - 1]])[rng.permutation(Cn)]
    cand[1] = [y[1], 3 if y[1] != 3 else 4, y[1], 3 if y[1] != 3 else 4, 7 if y[1] != 7 else 8, y[1]]
    cand[2] = [0, y[2], 0, 5 if y[2] != 5 else 6, 0, 0]
    cand[3] = [k for k in range(1, K + 1) if k != y[3]][:Cn]
    cand[4] = 0
    cand[5] = [0, 0, y[5], 0, 0, 0]
    if kind == "labels":
        ids, w = y[:, None].copy(), np.ones((B, 1), np.float32)
    else:
        ids = np.stack([y, rng.integers(0, K + 1, size=B), rng.integers(0, K + 1, size=B)], 1)
        w = rng.uniform(0.1, 1.0, size=(B, G)).astype(np.float32)
        ids[6] = [y[6], y[6], 0]                       # duplicates in the set add up
        ids[7, 0] = 0                                  # an empty first entry
    s = rng.uniform(0, 2, size=B).astype(np.float32)
    s[0] = 0.0
    return x, cand, ids, w, s


def torch_ce(x, cand, ids, w, s):
    """mean_b s_b sum_g w_g (logsumexp(x.gather(live)) - x[y_g]) over the kept entries, fp64 autograd"""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    rows = []
    for b in range(x.shape[0]):
        live = sorted({int(c) - 1 for c in cand[b] if c > 0})
        r = torch.zeros((), dtype=torch.float64)
        if live:
            lse = torch.logsumexp(xt[b].gather(0, torch.tensor(live)), 0)
            for g in range(ids.shape[1]):
                if ids[b, g] > 0 and ids[b, g] - 1 in live:
                    r = r + float(w[b, g]) * (lse - xt[b, ids[b, g] - 1])
        rows.append(float(s[b]) * r)
    rows = torch.stack(rows)
    rows.mean().backward()
    return rows.detach().numpy(), xt.grad.numpy()


def torch_bce(x, cand, ids, w, s):
    """mean_b s_b sum over the gathered columns of binary_cross_entropy_with_logits against the kept target"""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    rows = []
    for b in range(x.shape[0]):
        live = sorted({int(c) - 1 for c in cand[b] if c > 0})
        kept = [(int(ids[b, g]) - 1, float(w[b, g])) for g in range(ids.shape[1])
                if ids[b, g] > 0 and ids[b, g] - 1 in live]
        r = torch.zeros((), dtype=torch.float64)
        if kept:
            t = torch.tensor([min(1.0, sum(wg for k, wg in kept if k == c)) for c in live], dtype=torch.float64)
            r = torch.nn.functional.binary_cross_entropy_with_logits(xt[b].gather(0, torch.tensor(live)), t,
                                                                     reduction="sum")
        rows.append(float(s[b]) * r)
    rows = torch.stack(rows)
    rows.mean().backward()
    return rows.detach().numpy(), xt.grad.numpy()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(np.max(np.abs(b)), 1e-30))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["labels", "set"])
@pytest.mark.parametrize("crit", ["ce", "bce"])
def test_statements_against_fp64_autograd(crit, kind, weighted):
    x, cand, ids, w, s = case(kind)
    sw = s if weighted else None
    s_ref = s if weighted else np.ones(B)
    fwd, bwd, ref = {"ce": (predict.cand_ce, predict.cand_ce_grad, torch_ce),
                     "bce": (predict.cand_bce, predict.cand_bce_grad, torch_bce)}[crit]
    rows_ref, grad_ref = ref(x, cand, ids, w, s_ref)
    for dtype in (np.float64, np.float32):
        rows, mean = fwd(x, cand, ids, w, sw, dtype=dtype)
        grad = bwd(x, cand, ids, w, sw, dtype=dtype)
        assert rows.dtype == dtype and grad.dtype == dtype and grad.shape == x.shape
        print(crit, kind, dtype.__name__, rel(rows, rows_ref), rel(grad, grad_ref))
        assert rel(rows, rows_ref) < TOL and abs(float(mean) - rows_ref.mean()) < TOL * max(1.0, rows_ref.mean())
        assert rel(grad, grad_ref) < TOL
        # the row classes: nothing outside the live candidates, unlabelled rows are zero rows
        live = np.zeros((B, K), bool)
        for b in range(B):
            live[b, [c - 1 for c in cand[b] if c > 0]] = True
        assert np.all(grad[~live] == 0) and not np.signbit(grad[~live]).any()
        assert rows[3] == 0 and rows[4] == 0 and np.all(grad[3] == 0) and np.all(grad[4] == 0)
        if weighted:
            assert rows[0] == 0 and np.all(grad[0] == 0)          # s_b = 0
        if crit == "ce" and kind == "labels":
            assert abs(rows[5]) < 1e-6 and np.abs(grad[5]).max() < 1e-6     # the one live candidate is the truth


def test_live_and_kept():
    cand = np.array([[3, 0, 3, 5, 0, 5], [0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6]])
    assert predict.cand_live(cand).tolist() == [[True, False, False, True, False, False], [False] * 6, [True] * 6]
    ids = np.array([[3, 4, 0], [1, 0, 0], [6, 6, 7]])
    assert predict.cand_kept(cand, ids).tolist() == [[True, False, False], [False] * 3, [True, True, False]]
    labels = predict.cand_ce(np.zeros((3, 8), np.float32), cand, np.array([5, 1, 8]))      # labels as ids [B]
    assert labels[0][1] == 0 and labels[0][2] == 0 and abs(labels[0][0] - np.log(2)) < 1e-6


# ------------------------------------------------------------------------------------------ ranked candidates
def test_top_candidates_total_order_padding_and_the_multiply_rule():
    nan, inf = np.nan, np.inf
    x = np.array([[[0.5, 2.0, 2.0, -1.0, nan, -inf, 0.0, -0.0, 3.0, 1.0],
                   [-1.0, -2.0, -3.0, -0.5, -4.0, -5.0, -6.0, -7.0, -8.0, -9.0],
                   [1.0, 5.0, 2.0, 0.1, 0.2, 0.3, 9.0, 0.4, 0.5, 0.6]]], np.float32)
    cand = np.array([[3, 2, 5, 6, 8, 7, 2, 0],          # ties 2.0 (ids 2, 3), NaN, -inf, -0 / +0, a duplicate, an empty
                     [1, 2, 3, 0, 0, 0, 0, 0],          # all negative
                     [2, 4, 0, 0, 0, 0, 0, 0]])
    ids, score, conf = predict.top_candidates(x, cand, 8)
    assert ids[0, 0].tolist() == [2, 3, 7, 8, 6, 5, 0, 0]        # ties by the lower id, +0 == -0, NaN last, padding
    assert np.array_equal(score[0, 0, :4].view(np.uint32), x[0, 0, [1, 2, 6, 7]].view(np.uint32))
    assert score[0, 0, 4] == -inf and np.isnan(score[0, 0, 5])
    assert np.all(score[0, 0, 6:] == -inf) and np.all(conf[0, 0, 6:] == 0) and not np.signbit(conf[0, 0, 6:]).any()
    assert ids[0, 2].tolist() == [2, 4, 0, 0, 0, 0, 0, 0]
    e = np.exp(np.array([5.0, 0.1], np.float64) - 5.0)
    assert np.allclose(conf[0, 2, :2], e / e.sum(), rtol=1e-6) and abs(conf[0, 2, :2].sum() - 1) < 1e-6
    # rank 0 against the reference's multiply rule (predict.answers) on the finite rows: equal where the best
    # candidate is positive, different on the all-negative row, where a masked-out zero wins
    _oe, mc = predict.answers([x[0]], cand)
    assert mc[0, 2] == ids[0, 2, 0]
    assert ids[0, 1, 0] == 1 and mc[0, 1] == 4 and mc[0, 1] not in cand[1]
    with pytest.raises(ValueError):
        predict.top_candidates(x, cand, 9)
    with pytest.raises(ValueError):
        predict.top_candidates(x, cand, 0)
    with pytest.raises(ValueError):
        predict.top_candidates(x, cand + 10, 1)


def test_cand_stats_statement():
    rng = np.random.default_rng(3)
    H, n = 3, 6
    logits = rng.normal(size=(H, n, 10)).astype(np.float32)
    dopred = rng.uniform(size=(H, n)).astype(np.float32)
    dopred[:, 2] = 0.1                                              # no hop fires: the select row is the zero row
    y = np.array([1, 2, 3, 4, 5, 6])
    cand = np.stack([rng.permutation(10)[:4] + 1 for _ in range(n)])
    cand[:, 0] = y
    cand[4] = [7, 8, 9, 10]                                         # truth outside: unlabelled
    st = predict.cand_stats(logits, dopred, cand, y)
    assert st["n_lab"] == 5 and st["loss"].shape == (H + 2,) and st["ans"].shape == (H + 2, n)
    for h in range(H):
        assert st["loss"][h] == predict.cand_ce(logits[h], cand, y)[1]
        best = [cand[b][np.argmax(logits[h, b, cand[b] - 1])] for b in range(n)]
        assert st["ans"][h].tolist() == best
        assert st["correct"][h] == sum(best[b] == y[b] for b in range(n) if b != 4) == st["score"][h]
    assert st["ans"][H + 1, 2] == cand[2].min()                     # the zero row: ties go to the lower id
    sw = np.array([0, 1, 2, 1, 1, 0.5], np.float32)
    assert predict.cand_stats(logits, dopred, cand, y, sample_w=sw)["loss"][0] == \
        predict.cand_ce(logits[0], cand, y, None, sw)[1]
    bce = predict.cand_stats(logits, dopred, cand, y, loss="bce")
    assert bce["loss"][0] == predict.cand_bce(logits[0], cand, y)[1] and np.array_equal(bce["ans"], st["ans"])


# ------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_checks_shapes_and_ranges():
    from rau_vqa_amd.model import RAU

    class Stub:
        class cfg:
            K = 12
        MAX_CANDIDATES = RAU.MAX_CANDIDATES
    chk = lambda cand, n=4: RAU._candidates(Stub, cand, n)
    ok = chk(np.array([[1, 2, 0]] * 4))
    assert ok.dtype == np.int32 and ok.flags.c_contiguous and ok.shape == (4, 3)
    for bad in (np.zeros(4, int), np.zeros((3, 3), int), np.zeros((4, 0), int), np.zeros((4, 33), int),
                np.full((4, 3), 13), np.full((4, 3), -1)):
        with pytest.raises(ValueError):
            chk(bad)
    assert chk(np.full((4, 32), 12)).shape == (4, 32)
