"""The open hop recurrence (rau_set_state_dev, rau_state_dev, rau_backward_state, rau_state_grad_dev) on the host side:
the header, the ctypes table and the Lua shim declare the calls and the struct, the ABI version stays 5; and
tests/state_ref.py -- the oracle of tests/test_gpu_state.py -- checks itself: a chain of two segments against one run,
and the state gradient against a central finite difference.  No GPU."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import torch

from tests import ext_ref, state_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rau_set_state_dev": 4, "rau_batch_state": 2, "rau_state_dev": 3, "rau_backward_state": 7,
       "rau_state_grad_dev": 3, "rau_get_state_grad": 3}
FIELDS = ["d_h", "d_c_last"]
GROUPS = ("embed", "rnn", "mult")


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    return [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]


# ------------------------------------------------------------------------------------------ 1. declarations
def test_header_ctypes_and_lua_declare_the_calls_and_the_struct():
    from rau_vqa_amd import _lib
    header, lua = read("include", "rau.h"), read("bindings", "rau.lua")
    assert re.search(r"#define RAU_ABI_VERSION 5\b", header)
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    want = ["const float* " + f for f in FIELDS]
    assert struct_fields(header, "rau_state_grads") == want
    assert struct_fields(cdef, "rau_state_grads") == want
    assert [n for n, _ in _lib.RauStateGrads._fields_] == FIELDS
    assert C.sizeof(_lib.RauStateGrads) == 2 * C.sizeof(C.c_void_p)
    # rau_out_grads keeps its three fields
    assert struct_fields(header, "rau_out_grads") == ["const float* " + f for f in ("d_logits", "d_dopred", "d_attprob")]
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name, nargs in NEW.items():
        count = lambda text: len(re.search(r"\bint %s\s*\((.*?)\);" % name, text, flags=re.S).group(1).split(","))
        assert count(code) == count(cdef) == len(_lib._SIGS[name][1]) == nargs, name
        assert _lib._SIGS[name][0] is C.c_int
    for fn, call in (("setStateDev", "rau_set_state_dev"), ("stateDev", "rau_state_dev"),
                     ("backwardState", "rau_backward_state"), ("stateGrad", "rau_state_grad_dev")):
        assert "function RAU:%s(" % fn in lua and "C.%s(self.h" % call in lua, fn
    # the header says what is not offered
    doc = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header))
    for phrase in ("hops BEFORE the last is not offered", "no captured variant", "never accumulated"):
        assert phrase in doc, phrase


def test_python_has_the_methods():
    model, autograd = read("rau_vqa_amd", "model.py"), read("rau_vqa_amd", "autograd.py")
    for fn in ("set_state", "clear_state", "batch_state", "carry_state", "state_tensors", "state_grad",
               "state_grad_tensors"):
        assert "def %s(" % fn in model, fn
    assert re.search(r"def set_batch_dev\([^)]*state=None", model)
    assert re.search(r"def backward\([^)]*state_grads=None", model)
    assert re.search(r"def step\([^)]*state=None, return_state=False", autograd)


def test_the_library_exports_the_calls_and_checks_null():
    from rau_vqa_amd import _lib
    lib = _lib.lib()
    assert lib.rau_abi_version() == 5
    sg = _lib.RauStateGrads(None, None)
    assert lib.rau_set_state_dev(None, None, None, 0) == -1 and b"null" in lib.rau_last_error()
    assert lib.rau_batch_state(None, None) == -1
    assert lib.rau_state_dev(None, None, None) == -1
    assert lib.rau_backward_state(None, None, None, None, None, None, C.byref(sg)) == -1
    assert lib.rau_state_grad_dev(None, None, None) == -1
    assert lib.rau_get_state_grad(None, None, None) == -1


# ------------------------------------------------------------------------------------------ 2. the oracle
def problem(dims, H=None, seed=123):
    sh = util.shapes(dims) if H is None else util.shapes(dims, H=H)
    batch, params, masks = util.make_problem(sh, scale=0.5, seed=seed)
    return sh, batch, params, masks


def test_state_ref_from_zeros_is_ext_ref():
    """With an all-zero state and F blind to the states it is ext_ref.step (whose hop loop starts from zeros)."""
    sh, batch, params, masks = problem(util.SMALL)
    w = [3, 0.5, 2]
    G = np.random.default_rng(0).normal(size=(sh.H, sh.B, sh.K)) / sh.B
    z = np.zeros((sh.B, sh.R))
    a = ext_ref.step(sh, params, batch, masks, w, F=ext_ref.linear_F(G))
    b = state_ref.step(sh, params, batch, masks, w, z, z, F=state_ref.linear_F(G))
    for k in ("logits", "dopred", "att") + tuple("g_" + g for g in GROUPS):
        assert util.rel_err(b[k], a[k]) < 1e-12, k


def test_four_hops_equal_two_chained_runs_of_two():
    """Evaluate mode: an H = 4 run from (c0, h0) equals segment A (hops 1-2) followed by segment B (hops 3-4) from A's
    final state, in outputs, c, h, and -- with B's state gradient handed back to A as the gradient at its final state
    -- in the summed parameter gradients and the gradient at (c0, h0).  fp64 against fp64: 1e-10."""
    sh4, batch, params, _ = problem(util.SMALL, H=4)
    sh2 = dataclasses.replace(sh4, H=2)
    rng = np.random.default_rng(1)
    c0, h0 = 0.5 * rng.normal(size=(sh4.B, sh4.R)), np.tanh(rng.normal(size=(sh4.B, sh4.R)))
    w = [3.0, 0.5, 2.0, 1.0]
    G_h = rng.normal(size=(4, sh4.B, sh4.R)) / sh4.B
    G_c = rng.normal(size=(sh4.B, sh4.R)) / sh4.B
    whole = state_ref.step(sh4, params, batch, None, w, c0, h0, F=state_ref.linear_F(G_h=G_h, G_c_last=G_c))
    a_fwd = state_ref.step(sh2, params, batch, None, w[:2], c0, h0, backward=False)
    b = state_ref.step(sh2, params, batch, None, w[2:], a_fwd["c"][-1], a_fwd["h"][-1],
                       F=state_ref.linear_F(G_h=G_h[2:], G_c_last=G_c))
    Ga = G_h[:2].copy()
    Ga[-1] += b["d_h0"]
    a = state_ref.step(sh2, params, batch, None, w[:2], c0, h0, F=state_ref.linear_F(G_h=Ga, G_c_last=b["d_c0"]))
    for k in ("logits", "dopred", "att", "c", "h"):
        assert util.rel_err(np.concatenate([a[k], b[k]]), whole[k]) < 1e-10, k
    for g in GROUPS:
        assert util.rel_err(a["g_" + g] + b["g_" + g], whole["g_" + g]) < 1e-10, g
    for k in ("d_c0", "d_h0"):
        assert np.abs(whole[k]).max() > 0 and util.rel_err(a[k], whole[k]) < 1e-10, k


def test_state_gradient_against_a_central_finite_difference():
    """d_c0 / d_h0 at util.EDGE (H = 1, train-mode masks): every element against (L(x + e) - L(x - e)) / 2e in fp64."""
    sh, batch, params, masks = problem(util.EDGE)
    rng = np.random.default_rng(2)
    c0, h0 = 0.5 * rng.normal(size=(sh.B, sh.R)), np.tanh(rng.normal(size=(sh.B, sh.R)))
    G_h = rng.normal(size=(sh.H, sh.B, sh.R))
    G_c = rng.normal(size=(sh.B, sh.R))
    F = state_ref.linear_F(G_h=G_h, G_c_last=G_c)
    w = [1.5]
    y = torch.as_tensor(batch["labels"]).long() - 1

    def value(c, h):
        r = state_ref.step(sh, params, batch, masks, w, c, h, F=F, backward=False)
        ce = torch.nn.functional.cross_entropy(torch.as_tensor(r["logits"][0]), y)
        return w[0] * float(ce) + r["ext"]

    ref = state_ref.step(sh, params, batch, masks, w, c0, h0, F=F)
    eps = 1e-6
    for key, which in (("d_c0", 0), ("d_h0", 1)):
        fd = np.zeros((sh.B, sh.R))
        for i in range(sh.B):
            for j in range(sh.R):
                d = np.zeros((sh.B, sh.R))
                d[i, j] = eps
                args = lambda s: (c0 + s * d, h0) if which == 0 else (c0, h0 + s * d)
                fd[i, j] = (value(*args(1)) - value(*args(-1))) / (2 * eps)
        assert np.abs(ref[key]).max() > 1e-3
        # central difference: truncation O(eps^2) and cancellation ~1e-16 / eps on values of order 1
        assert util.rel_err(fd, ref[key]) < 1e-7, (key, util.rel_err(fd, ref[key]))


def test_state_ref_region_counts_slice_the_leaves():
    """Per-sample runs hang on the same state leaves: the gradient rows are those of the samples."""
    sh, batch, params, masks = problem(util.EDGE)
    rng = np.random.default_rng(3)
    c0, h0 = 0.5 * rng.normal(size=(sh.B, sh.R)), np.tanh(rng.normal(size=(sh.B, sh.R)))
    full = np.full(sh.B, sh.S, np.int32)
    a = state_ref.step(sh, params, batch, masks, [1.0], c0, h0)
    b = state_ref.step(sh, params, batch, masks, [1.0], c0, h0, nreg=full)
    for k in ("logits", "att", "c", "h", "d_c0", "d_h0", "g_mult"):
        assert util.rel_err(b[k], a[k]) < 1e-10, k
