"""The merged answers as training terms (rau_backward_merged) on the host side: joint.merged_ce_grad -- the numpy
statement of what the device adds to d_logits -- against torch autograd of the two merged cross-entropies, and the
header, the Lua shim and the ctypes table declare and call the three new entry points.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from rau_vqa_amd import joint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rau_backward_merged", "rau_graph_step_merged", "rau_merge_criterion_backward")
H, B, K = 3, 9, 12


def problem(seed=0, H=H, B=B, K=K):
    """Random logits and do_pred with every kind of row: rows 0, 1 never fire, row 2 fires at hop 0 (and again
    later), row 3 first fires at the last hop; the others as drawn."""
    rng = np.random.default_rng(seed)
    lg = rng.normal(size=(H, B, K))
    dp = rng.uniform(size=(H, B))
    dp[:, :2] = rng.uniform(0.0, 0.5, size=(H, 2))
    dp[:, 2] = 0.9
    if H > 1:
        dp[:, 3] = 0.1
        dp[H - 1, 3] = 0.8
    y = rng.integers(1, K + 1, size=B)
    return lg, dp, y


def answer_set(rng, B, K, y):
    ids = rng.integers(1, K + 1, size=(B, 3))
    ids[:, 0] = y
    w = rng.uniform(0.1, 1.0, size=(B, 3))
    ids[1, :] = 0              # an unlabelled row
    ids[4, 2] = ids[4, 0]      # duplicates add up
    ids[5, 1] = 0              # an empty entry whose weight is ignored
    return ids, w


def autograd(lg, dp, merge_w, y=None, answers=None):
    """d( w_uni CE(mean_h l_h) + w_sel CE(sum_h l_h gate_h) ) / d l in fp64, gate = the detached first-fire indicator"""
    t = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
    nH, nB = dp.shape
    gate = np.zeros((nH, nB))
    did = np.zeros(nB, bool)
    for h in range(nH):
        do = dp[h] > 0.5
        gate[h] = do & ~did
        did |= do
    g = torch.tensor(gate)
    uni = t.mean(0)
    sel = (t * g[:, :, None]).sum(0)
    if answers is None:
        yy = torch.tensor(np.asarray(y) - 1)
        ce = lambda r: torch.nn.functional.cross_entropy(r, yy)
    else:
        ids = torch.tensor(answers[0]).long()
        aw = torch.where(ids > 0, torch.tensor(answers[1], dtype=torch.float64), torch.zeros((), dtype=torch.float64))
        ce = lambda r: (aw * (torch.logsumexp(r, 1, keepdim=True) - torch.gather(r, 1, (ids - 1).clamp(min=0)))).sum() / nB
    (merge_w[0] * ce(uni) + merge_w[1] * ce(sel)).backward()
    return t.grad.numpy(), gate


@pytest.mark.parametrize("merge_w", [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)])
def test_float64_statement_equals_autograd_with_labels(merge_w):
    lg, dp, y = problem()
    ref, gate = autograd(lg, dp, merge_w, y=y)
    got = joint.merged_ce_grad(lg, dp, labels=y, merge_w=merge_w)
    assert got.dtype == np.float64 and got.shape == lg.shape
    assert np.max(np.abs(got - ref)) < 1e-10
    assert gate.sum(0).min() == 0 and gate[0].sum() > 0 and gate[1:].sum() > 0   # every kind of row occurred


@pytest.mark.parametrize("merge_w", [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)])
def test_float64_statement_equals_autograd_with_an_answer_set(merge_w):
    lg, dp, y = problem(seed=1)
    ans = answer_set(np.random.default_rng(2), B, K, y)
    ref, _gate = autograd(lg, dp, merge_w, answers=ans)
    got = joint.merged_ce_grad(lg, dp, answers=ans, merge_w=merge_w)
    assert np.max(np.abs(got - ref)) < 1e-10
    assert np.all(got[:, 1] == 0)   # the unlabelled row: zero gradient in both terms


def test_rows_without_a_firing_hop_are_exactly_zero_in_the_select_term():
    lg, dp, y = problem()
    for dt in (np.float64, np.float32):
        got = joint.merged_ce_grad(lg.astype(dt), dp, labels=y, merge_w=(0.0, 1.3))
        assert got.dtype == dt
        assert np.all(got[:, :2] == 0)                  # rows 0, 1 never fire
        assert np.all(got[1:, 2] == 0) and np.any(got[0, 2] != 0)      # row 2: hop 0 only, though it fires again
        assert np.all(got[:H - 1, 3] == 0) and np.any(got[H - 1, 3] != 0)
    _uni, select, hsel = joint.merged_rows(lg, dp)
    assert list(hsel[:4]) == [-1, -1, 0, H - 1] and np.all(select[:2] == 0)
    assert np.array_equal(select[2], lg[0, 2]) and np.array_equal(select[3], lg[H - 1, 3])


def test_one_hop_uni_is_the_hops_own_criterion_gradient():
    lg, dp, y = problem(seed=3, H=1)
    got = joint.merged_ce_grad(lg, dp, labels=y, merge_w=(1.0, 0.0))
    t = torch.tensor(lg[0], requires_grad=True)
    torch.nn.functional.cross_entropy(t, torch.tensor(y - 1)).backward()
    assert np.max(np.abs(got[0] - t.grad.numpy())) < 1e-10


def test_float32_statement_follows_the_float64_one_and_the_merge_lines_of_feval_stats():
    lg, dp, y = problem(seed=4)
    lg32 = lg.astype(np.float32)
    g64 = joint.merged_ce_grad(lg32.astype(np.float64), dp, labels=y, merge_w=(0.7, 1.3))
    g32 = joint.merged_ce_grad(lg32, dp, labels=y, merge_w=(0.7, 1.3))
    assert g32.dtype == np.float32 and np.max(np.abs(g32 - g64)) < 1e-6
    # the rows are the ones feval_stats takes the logged losses of
    uni, select, _hsel = joint.merged_rows(lg32, dp)
    st = joint.feval_stats(lg32, dp.astype(np.float32), y)
    assert joint.cross_entropy(uni, y) == st["loss"][H] and joint.cross_entropy(select, y) == st["loss"][H + 1]
    with pytest.raises(ValueError):
        joint.merged_ce_grad(lg, dp, merge_w=(1, 1))


def test_header_declares_the_three_entry_points_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "rau.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, code), name
    assert "#define RAU_ABI_VERSION 5" in header


def test_lua_shim_declares_what_it_calls():
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    body = lua.replace(cdef, "")
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, cdef), name
    for name in NEW[:2]:
        assert "C.%s(" % name in body, name
    assert "function RAU:backward(hop_w, select_w, att_w, merge_w)" in body
    assert re.search(r"function RAU:graphStep\([^)]*merge_w\)", body)
    called = set(re.findall(r"\bC\.(rau_[a-z_0-9]+)\(", body))
    declared = set(re.findall(r"\b(rau_[a-z_0-9]+)\s*\(", cdef))
    assert called <= declared, sorted(called - declared)


def test_python_binding_table_declares_the_three_symbols():
    from rau_vqa_amd import _lib
    assert len(_lib._SIGS["rau_backward_merged"][1]) == 5
    assert len(_lib._SIGS["rau_graph_step_merged"][1]) == 6
    assert len(_lib._SIGS["rau_merge_criterion_backward"][1]) == 6
