"""Host side of the step-selection head's gradient (rau_backward_select): joint.bce_grad / joint.select_signal,
the numpy statement of the contract in include/rau.h, and the Lua shim's declarations."""
import os
import re

import numpy as np
import torch

from rau_vqa_amd import joint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(joint.BCE_EPS)


def autograd(x, t, w):
    """d/dx and d/dz (x = sigmoid(z)) of  sum_h w[h] * mean_b eps-BCE(x[h,b], t[h,b])  in fp64."""
    z = torch.logit(torch.as_tensor(x, dtype=torch.float64)).requires_grad_(True)
    xs = torch.sigmoid(z)
    xs.retain_grad()
    tt = torch.as_tensor(t, dtype=torch.float64)
    bce = -(tt * torch.log(xs + EPS) + (1 - tt) * torch.log(1 - xs + EPS)).mean(dim=1)
    (torch.as_tensor(w, dtype=torch.float64) * bce).sum().backward()
    return xs.grad.numpy(), z.grad.numpy()


def test_bce_grad_and_select_signal_against_autograd():
    """To 1e-12, absolute.  nn.BCECriterion's backward is not exactly the derivative of its forward: the two
    differ by w/n * eps (2t - 1) / ((1 - x + eps)(x + eps)).  With n = 64, w <= 2 and x in [0.1, 0.9] that term
    is at most 2/64 * 1e-12 / 0.09 = 3.5e-13; fp64 rounding of values below 1 adds ~1e-16."""
    rng = np.random.RandomState(0)
    H, n = 3, 64
    x = rng.uniform(0.1, 0.9, size=(H, n))
    t = (rng.uniform(size=(H, n)) < 0.4).astype(np.float64)
    w = np.array([0.7, 0.0, 2.0])
    dx, dz = autograd(x, t, w)
    g, s = joint.bce_grad(x, t, w), joint.select_signal(x, t, w)
    assert g.dtype == np.float64 and s.dtype == np.float64
    assert np.max(np.abs(g - dx)) < 1e-12
    assert np.max(np.abs(s - dz)) < 1e-12
    assert not g[1].any() and g[0].any() and g[2].any()
    # a scalar weight on one hop's row is the same statement
    assert np.array_equal(joint.bce_grad(x[2], t[2], 2.0), g[2])
    # float32 inputs: the device's arithmetic, float32 out, within a few ulp of the fp64 statement
    g32 = joint.bce_grad(x.astype(np.float32), t, w)
    s32 = joint.select_signal(x.astype(np.float32), t, w)
    assert g32.dtype == np.float32 and s32.dtype == np.float32
    x32 = x.astype(np.float32).astype(np.float64)
    assert np.allclose(g32, joint.bce_grad(x32, t, w), rtol=1e-6, atol=0)
    assert np.allclose(s32, joint.select_signal(x32, t, w), rtol=1e-6, atol=0)


def test_saturated_do_pred_is_finite_and_gives_no_signal():
    one, zero = np.float32(1), np.float32(0)
    x = np.array([zero, one, np.nextafter(zero, one), np.nextafter(one, zero)], np.float32)
    for tv in (0.0, 1.0):
        t = np.full(4, tv, np.float32)
        g, s = joint.bce_grad(x, t, 3.0), joint.select_signal(x, t, 3.0)
        assert g.dtype == np.float32 and np.all(np.isfinite(g)) and np.all(np.isfinite(s))
        assert s[0] == 0 and s[1] == 0          # x exactly 0 or 1: x (1 - x) = 0 kills the 1/eps
    # the sign: towards the target
    assert joint.bce_grad(x[2:], np.ones(2, np.float32), 1.0).max() < 0
    assert joint.bce_grad(x[2:], np.zeros(2, np.float32), 1.0).min() > 0


def test_torch_tensors_pass_through():
    x = torch.tensor([0.2, 0.6, 0.9], dtype=torch.float32)
    t = torch.tensor([1.0, 0.0, 1.0])
    g = joint.bce_grad(x, t, 1.5)
    assert isinstance(g, torch.Tensor) and g.dtype == torch.float32
    assert np.allclose(g.numpy(), joint.bce_grad(x.numpy(), t.numpy(), 1.5), rtol=1e-6, atol=0)


def test_lua_shim_declares_and_calls_both_entry_points():
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    body = lua.replace(cdef, "")
    for name in ("rau_backward_select", "rau_graph_step_select"):
        assert re.search(r"\bint %s\(" % name, cdef), name
        assert "C.%s(" % name in body, name
    # select_w is backward's second argument (the one method also takes the later terms behind it)
    assert "function RAU:graphStep(" in body and re.search(r"function RAU:backward\(hop_w, select_w[,)]", body)


def test_python_binding_table_lists_both_entry_points():
    from rau_vqa_amd import _lib
    assert len(_lib._SIGS["rau_backward_select"][1]) == 3
    assert len(_lib._SIGS["rau_graph_step_select"][1]) == 4
