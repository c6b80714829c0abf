"""The caller's attention bias (rau_set_att_bias_dev, rau_att_bias_grad_dev, rau_multimodal_forward_bias) on the host
side: the header, the ctypes table and the Lua shim declare the five calls, the ABI version stays 5; tests/bias_ref.py
-- the oracle of tests/test_gpu_att_bias.py -- checks itself against a central finite difference; and the check that
RAU.set_att_bias runs on numpy input refuses what it must, without a device.  No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import bias_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rau_set_att_bias_dev": 3, "rau_batch_att_bias": 2, "rau_att_bias_grad_dev": 3, "rau_get_att_bias_grad": 2,
       "rau_multimodal_forward_bias": 13}


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ------------------------------------------------------------------------------------------ 1. declarations
def test_header_ctypes_and_lua_declare_the_five_calls():
    from rau_vqa_amd import _lib
    header, lua = read("include", "rau.h"), read("bindings", "rau.lua")
    assert re.search(r"#define RAU_ABI_VERSION 5\b", header)
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name, nargs in NEW.items():
        count = lambda text: len(re.search(r"\bint %s\s*\((.*?)\);" % name, text, flags=re.S).group(1).split(","))
        assert count(code) == count(cdef) == len(_lib._SIGS[name][1]) == nargs, name
        assert _lib._SIGS[name][0] is C.c_int
    # rau_multimodal_forward_regions plus one pointer
    assert len(_lib._SIGS["rau_multimodal_forward_bias"][1]) == len(_lib._SIGS["rau_multimodal_forward_regions"][1]) + 1
    for fn, call in (("setAttBiasDev", "rau_set_att_bias_dev"), ("attBiasGrad", "rau_att_bias_grad_dev")):
        assert "function RAU:%s(" % fn in lua and "C.%s(self.h" % call in lua, fn
    # the header says what a row without a finite entry gives, and what is not offered
    doc = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header))
    for phrase in ("attention row is then NaN", "a bias per hop", "asynchronous upload slots",
                   "the gradient at module level", "an external gradient AT the bias", "never accumulated"):
        assert phrase in doc, phrase


def test_python_has_the_methods():
    model, autograd = read("rau_vqa_amd", "model.py"), read("rau_vqa_amd", "autograd.py")
    for fn in ("set_att_bias", "set_att_mask", "clear_att_bias", "batch_att_bias", "att_bias_grad",
               "att_bias_grad_tensor", "check_att_bias"):
        assert "def %s(" % fn in model, fn
    assert re.search(r"def set_batch_dev\([^)]*att_bias=None", model)
    assert re.search(r"def step\([^)]*\*,[^)]*att_bias=None", autograd)          # keyword-only


def test_the_library_exports_the_calls_and_checks_null():
    from rau_vqa_amd import _lib
    lib = _lib.lib()
    assert lib.rau_abi_version() == 5
    assert lib.rau_set_att_bias_dev(None, None, 0) == -1 and b"null" in lib.rau_last_error()
    assert lib.rau_batch_att_bias(None, None) == -1
    assert lib.rau_att_bias_grad_dev(None, None, None) == -1
    assert lib.rau_get_att_bias_grad(None, None) == -1
    assert lib.rau_multimodal_forward_bias(None, 0, *[None] * 11) == -1


# ------------------------------------------------------------------------------------------ 2. the oracle
HOP_W = [3.0, 0.5, 2.0]


@functools.lru_cache(maxsize=None)
def small():
    sh = util.shapes(util.SMALL)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    bias = bias_ref.pattern(sh.B, sh.S)
    n = np.array([12, 7, 12, 12, 5, 12, 2, 9], np.int32)      # ragged counts on the rows that can bear them
    return sh, batch, params, masks, bias, n


@functools.lru_cache(maxsize=None)
def small_ref(with_counts):
    sh, batch, params, masks, bias, n = small()
    return bias_ref.step(sh, params, batch, masks, HOP_W, bias, n if with_counts else None)


def objective(bias, n):
    sh, batch, params, masks, _, _ = small()
    r = bias_ref.step(sh, params, batch, masks, HOP_W, bias, n)
    return float(np.dot(HOP_W, r["losses"]))


@pytest.mark.parametrize("with_counts", [False, True])
def test_bias_ref_gradient_against_a_central_finite_difference(with_counts):
    """sum_h hop_w[h] loss_h, train-mode masks, fp64: a central difference in two bias entries -- the largest gradient
    entries of a random row and of the alternately masked row -- equals d_bias to 1e-6 relative."""
    sh, batch, params, masks, bias, n = small()
    n = n if with_counts else None
    d = small_ref(with_counts)["d_bias"]
    assert d.shape == (sh.B, sh.S)
    eps = 1e-5   # truncation ~eps^2, cancellation ~1e-16 L / eps: both far below 1e-6 of a gradient of order 1e-3
    for b in (5, 1):
        s = int(np.argmax(np.abs(d[b])))
        assert np.isfinite(bias[b, s]) and abs(d[b, s]) > 1e-5
        hi, lo = bias.astype(np.float64), bias.astype(np.float64)
        hi[b, s] += eps
        lo[b, s] -= eps
        fd = (objective(hi, n) - objective(lo, n)) / (2 * eps)
        print(b, s, fd, d[b, s])
        assert abs(fd - d[b, s]) <= 1e-6 * abs(d[b, s]), (b, s, fd, d[b, s])


@pytest.mark.parametrize("with_counts", [False, True])
def test_bias_ref_rows_sum_to_zero_and_masked_entries_are_zero(with_counts):
    sh, batch, params, masks, bias, n = small()
    r = small_ref(with_counts)
    d = r["d_bias"]
    assert np.abs(d).max() > 1e-4
    assert np.all(np.abs(d.sum(axis=1)) < 1e-12), d.sum(axis=1)
    masked = np.isneginf(bias)
    if with_counts:
        masked |= np.arange(sh.S)[None, :] >= n[:, None]
    assert np.all(d[masked] == 0)
    assert np.all(r["att"][:, masked] == 0)
    assert np.all(r["att"][:, 0, 2] == 1.0)                   # the row with one finite position
    assert np.all(d[0] == 0)                                  # ... has no gradient: its softmax is a constant


def test_bias_ref_minus_inf_is_minus_1e30_and_zero_bias_is_the_oracle():
    import oracle
    sh, batch, params, masks, bias, n = small()
    as_big = np.where(np.isneginf(bias), -1e30, bias.astype(np.float64))
    a, b = small_ref(False), bias_ref.step(sh, params, batch, masks, HOP_W, as_big)
    for k in ("att", "logits", "d_bias", "g_mult"):
        assert np.array_equal(a[k], b[k]) and np.isfinite(a[k]).all(), k
    plain = oracle.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks,
                        np.asarray(HOP_W, np.float32), dtype=np.float64)
    zero = bias_ref.step(sh, params, batch, masks, HOP_W, np.zeros((sh.B, sh.S), np.float32))
    for k in ("logits", "att", "g_mult", "g_rnn", "g_embed"):
        assert util.rel_err(zero[k], plain[k]) < 1e-10, k


# ------------------------------------------------------------------------------------------ 3. refusals, no device
def test_check_att_bias_refuses_what_the_device_cannot_check():
    from rau_vqa_amd.model import check_att_bias
    B, S = 4, 6
    good = bias_ref.pattern(B, S, edge=3)
    out = check_att_bias(good, B, S)
    assert out.dtype == np.float32 and out.flags.c_contiguous and np.array_equal(out, good)
    assert check_att_bias(good.astype(np.float64), B, S).dtype == np.float32
    for bad_value, word in ((np.nan, "NaN"), (np.inf, r"\+inf")):
        bad = good.copy()
        bad[1, 2] = bad_value
        with pytest.raises(ValueError, match=word):
            check_att_bias(bad, B, S)
    empty = good.copy()
    empty[3] = -np.inf
    with pytest.raises(ValueError, match=r"rows \[3\]"):
        check_att_bias(empty, B, S)
    behind = good.copy()                                       # finite only behind its region count
    behind[1, :4] = -np.inf
    check_att_bias(behind, B, S)
    check_att_bias(behind, B, S, regions=[6, 5, 6, 6])
    with pytest.raises(ValueError, match=r"rows \[1\].*region count"):
        check_att_bias(behind, B, S, regions=[6, 4, 6, 6])
    for wrong in (good[:3], good[:, :5], np.zeros((B, S), np.int32)):
        with pytest.raises(ValueError):
            check_att_bias(wrong, B, S)
    with pytest.raises(ValueError):
        check_att_bias(good, B, S, regions=[6, 0, 6, 6])


def test_set_att_bias_raises_before_anything_is_uploaded():
    """RAU.set_att_bias on numpy input runs the check first: with no context behind the object the refusals are
    reached, an upload would not be."""
    from rau_vqa_amd.model import RAU, Config
    m = object.__new__(RAU)
    m.cfg, m._n, m._h = Config(B=4, S=6), 4, None
    good = bias_ref.pattern(4, 6, edge=3)
    for bad in (np.where(np.arange(6) == 1, np.nan, good).astype(np.float32),
                np.where(np.arange(6) == 1, np.inf, good).astype(np.float32),
                np.full((4, 6), -np.inf, np.float32)):
        with pytest.raises(ValueError):
            m.set_att_bias(bad)
    behind = good.copy()
    behind[1, :4] = -np.inf
    with pytest.raises(ValueError, match="region count"):
        m.set_att_bias(behind, regions=np.array([6, 4, 6, 6]))
    with pytest.raises(ValueError):
        m.set_att_mask(np.zeros((4, 6), bool))


@pytest.mark.parametrize("with_counts", [False, True])
def test_the_two_references_agree(with_counts):
    """bias_ref.torch_step (the bias as a leaf of ref_torch) against bias_ref.step (the flat oracle, per sample): fp64
    against fp64, 1e-10."""
    sh, batch, params, masks, bias, n = small()
    a = small_ref(with_counts)
    b = bias_ref.torch_step(sh, params, batch, masks, HOP_W, bias, n if with_counts else None)
    for k in ("logits", "att", "dopred", "losses", "att_c", "att_h", "g_mult", "g_rnn", "g_embed", "d_bias"):
        assert util.rel_err(b[k], a[k]) < 1e-10, k
