"""Attention supervision, host side: the numpy statement (joint.att_ce / att_ce_grad / att_stats), the header,
Python argument validation and the reference of the GPU tests (tests/att_ref.py).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_torch
from rau_vqa_amd import joint
from tests import att_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def problem(H=3, B=6, S=13, seed=0):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(H, B, S))
    a = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    t = rng.uniform(0, 1, size=(B, S)) * (rng.uniform(size=(B, S)) < 0.6)
    t[1] = 0
    w = np.array([0.5, 3.0, 1.5])[:H]
    nreg = np.array([13, 5, 1, 12, 7, 13])[:B]
    return a, t, w, nreg


@pytest.mark.parametrize("counts", [False, True])
def test_grad_is_autograd_of_the_loss_in_float64(counts):
    a, t, w, nreg = problem()
    n = nreg if counts else None
    at = torch.tensor(a, requires_grad=True)
    live = torch.ones(a.shape[1:], dtype=torch.bool) if n is None else \
        torch.arange(a.shape[2])[None, :] < torch.tensor(n)[:, None]
    loss = ((torch.tensor(t) * live) * -torch.log(at + 1e-12)).sum((1, 2)) / a.shape[1]
    (torch.tensor(w) * loss).sum().backward()
    got = joint.att_ce_grad(a, t, w, n)
    assert got.dtype == np.float64
    assert util.rel_err(got, at.grad.numpy()) < 1e-12
    assert util.rel_err(joint.att_ce(a, t, n), loss.detach().numpy()) < 1e-12


def test_zero_rows_counts_and_the_float32_order():
    a, t, w, nreg = problem()
    g = joint.att_ce_grad(a.astype(np.float32), t, w, nreg)
    assert g.dtype == np.float32
    assert not g[:, 1].any()                                        # an all-zero row: no gradient
    for b, nb in enumerate(nreg):
        assert not g[:, b, nb:].any(), b                            # behind the count: none either
    z = (t == 0) | (np.arange(t.shape[1])[None, :] >= nreg[:, None])
    assert np.array_equal(np.signbit(g[:, z]), np.zeros_like(g[:, z], bool))   # exactly +0
    # the contract's order, every operation rounded once in float32
    f = np.float32
    a32, t32 = a.astype(f), t.astype(f)
    for h in range(3):
        want = -((f(w[h]) * t32) / (a32[h] + f(1e-12))) / f(a.shape[1])
        assert np.array_equal(g[h][~z], want[~z])
    # huge finite values behind the counts change nothing
    t2 = t.copy()
    for b, nb in enumerate(nreg):
        t2[b, nb:] = 3e38
    assert np.array_equal(joint.att_ce_grad(a.astype(f), t2, w, nreg), g)
    assert np.array_equal(joint.att_ce(a, t2, nreg), joint.att_ce(a, t, nreg))
    # finite at a == 0
    assert np.isfinite(joint.att_ce_grad(np.zeros((1, 2, 3), f), np.ones((2, 3), f), 1.0)).all()


def test_att_stats_statement():
    a, t, _w, nreg = problem()
    st = joint.att_stats(a, t, nreg)
    live = np.arange(t.shape[1])[None, :] < nreg[:, None]
    pos = (t > 0) & live
    sup = pos.any(1)
    assert st["n_sup"] == int(sup.sum()) and not sup[1]
    for h in range(a.shape[0]):
        loss = sum(t[b, s] * -np.log(a[h, b, s] + 1e-12) for b in range(a.shape[1]) for s in range(nreg[b]))
        assert abs(st["loss"][h] - loss / a.shape[1]) < 1e-12
        mass = np.mean([a[h, b][pos[b]].sum() for b in np.flatnonzero(sup)])
        assert abs(st["mass"][h] - mass) < 1e-12
        hits = sum(bool(pos[b, np.argmax(a[h, b, :nreg[b]])]) for b in np.flatnonzero(sup))
        assert st["hits"][h] == hits
    none = joint.att_stats(a, np.zeros_like(t))
    assert none["n_sup"] == 0 and not none["loss"].any() and not none["mass"].any() and not none["hits"].any()


def test_header_declares_the_calls_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "rau.h")).read()
    assert re.search(r"^#define RAU_ABI_VERSION 5$", text, flags=re.M)
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for proto in (
            "int rau_set_att_targets(rau_ctx* ctx, int slot, const float* t );",
            "int rau_batch_att_targets(rau_ctx* ctx, int* has);",
            "int rau_backward_att(rau_ctx* ctx, const float* hop_w, const float* select_w , const float* att_w );",
            "int rau_graph_step_att(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w, "
            "int zero_grads_first);",
            "int rau_att_stats(rau_ctx* ctx, float* loss , float* mass , int32_t* hits , int32_t* n_sup);",
            "int rau_att_criterion_forward(rau_ctx* ctx, int h, const float* attprob_dev , const float* t_dev , "
            "const int32_t* nreg_dev , float* loss);",
            "int rau_att_criterion_backward(rau_ctx* ctx, int h, const float* attprob_dev, const float* t_dev, "
            "const int32_t* nreg_dev, float scale, float** d_attprob );"):
        assert proto in code, proto


class _NoLibrary:
    """RAU's host-side checks run before anything reaches the library."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


def test_python_validates_targets_before_the_library():
    from rau_vqa_amd.model import RAU, Config
    m = RAU.__new__(RAU)
    m.cfg, m._n, m._lib, m._h = Config(B=4, S=6), 4, _NoLibrary(), None
    good = np.ones((4, 6), np.float32)
    assert m._att_targets(good, 4).shape == (4, 6)
    assert m._att_targets(np.ones((4, 2, 3)), 4).shape == (4, 6)     # a [B, W, H] map
    bad_shape, negative, nan, inf = np.ones((3, 6)), good.copy(), good.copy(), good.copy()
    negative[1, 2], nan[0, 0], inf[3, 5] = -1e-3, np.nan, np.inf
    for bad in (bad_shape, np.ones((4, 5)), np.ones(24), negative, nan, inf):
        with pytest.raises(ValueError):
            m.set_att_targets(bad)
        with pytest.raises(ValueError):
            m.set_batch(None, None, np.ones(4, np.int32), att_targets=bad)
        with pytest.raises(ValueError):
            m.set_batch_async(0, att_targets=bad)
    with pytest.raises(ValueError):
        m.backward(np.ones(8), att_w=np.ones(3))
    m._h = None


def test_reference_without_the_term_is_ref_torch_step():
    sh = util.shapes(util.SMALL)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    hop_w = np.full(sh.H, float(sh.H))
    want = ref_torch.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks, hop_w)
    t = att_ref.targets(want["att"])
    assert att_ref.check(want["att"], t)
    for got in (att_ref.step(sh, params, batch, masks, hop_w),
                att_ref.step(sh, params, batch, masks, hop_w, [0, 0, 0], t),
                att_ref.step(sh, params, batch, masks, hop_w, [0, 0, 0], t, nreg=np.full(sh.B, sh.S))):
        for k in util.OUT_KEYS + util.GRAD_KEYS:
            assert util.rel_err(got[k], want[k]) < 1e-9, k
        assert np.array_equal(got["argmax"], want["argmax"])
    # and with the term: the reported loss is joint.att_ce of the oracle's own attention, the gradients move
    w = [0.5, 3, 1.5]
    with_term = att_ref.step(sh, params, batch, masks, hop_w, w, t)
    assert util.rel_err(with_term["att_losses"], joint.att_ce(want["att"], t)) < 1e-12
    assert util.rel_err(with_term["g_mult"], want["g_mult"]) > 1e-3
    # per-sample runs with mixed counts: the attention is zero behind them, and the loss ignores targets there
    n = np.array([12, 7, 3, 1, 5, 12, 2, 9])
    counted = att_ref.step(sh, params, batch, masks, hop_w, w, t, nreg=n)
    for b, nb in enumerate(n):
        assert not counted["att"][:, b, nb:].any()
    assert util.rel_err(counted["att_losses"], joint.att_ce(counted["att"], t, n)) < 1e-12
