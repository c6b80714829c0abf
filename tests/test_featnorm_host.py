"""Host side of the per-position L2 normalisation (rau_set_feat_norm): the numpy statements, the header, the exports."""
import ctypes as C
import os
import re

import numpy as np
import torch

from rau_vqa_amd import _lib, feat16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rau_set_feat_norm", "rau_feat_norm", "rau_norm_feats_dev", "rau_get_norm_feats", "rau_dev_l2norm",
         "rau_dev_l2norm_backward")
EPS = 1e-3


def maps(D=12, S=7, n=3, seed=0):
    """Maps with one all-zero position and one position of norm 1e-5 < EPS; every other norm is far above EPS."""
    x = np.random.default_rng(seed).normal(size=(n, D, S)).astype(np.float32)
    x[0, :, 2] = 0.0
    x[1, :, 4] *= np.float32(1e-5 / np.sqrt(np.sum(x[1, :, 4].astype(np.float64) ** 2)))
    return x


def test_l2_normalize_is_torch_normalize_in_float64():
    x = maps()
    ref = torch.nn.functional.normalize(torch.as_tensor(x.astype(np.float64)), p=2.0, dim=1, eps=EPS).numpy()
    got = feat16.l2_normalize(x, EPS)
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got, ref.astype(np.float32))
    assert np.all(got[0, :, 2] == 0) and not np.any(np.signbit(got[0, :, 2]))
    # under eps the forward is x / eps
    assert np.array_equal(got[1, :, 4], (x[1, :, 4].astype(np.float64) / EPS).astype(np.float32))
    # the default eps
    ref0 = torch.nn.functional.normalize(torch.as_tensor(x.astype(np.float64)), p=2.0, dim=1).numpy()
    assert np.array_equal(feat16.l2_normalize(x), ref0.astype(np.float32))


def test_l2_normalize_grad_is_autograd_through_normalize():
    x = maps(seed=1)
    g = np.random.default_rng(2).normal(size=x.shape).astype(np.float32)
    t = torch.as_tensor(x.astype(np.float64)).requires_grad_(True)
    y = torch.nn.functional.normalize(t, p=2.0, dim=1, eps=EPS)
    (y * torch.as_tensor(g.astype(np.float64))).sum().backward()
    ref = t.grad.numpy()
    got = feat16.l2_normalize_grad(x, g, EPS)
    assert got.dtype == np.float32 and got.shape == x.shape
    # two float64 evaluations of one formula, rounded to float32: equal to an ulp of float32 at the largest entry
    assert np.max(np.abs(got.astype(np.float64) - ref)) <= 2.0 ** -23 * np.max(np.abs(ref))
    # the linear branch: g / eps, and on the zero position too
    for n, s in ((1, 4), (0, 2)):
        assert np.array_equal(got[n, :, s], (g[n, :, s].astype(np.float64) / EPS).astype(np.float32))


def header():
    text = open(os.path.join(ROOT, "include", "rau.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_calls_and_keeps_the_abi_version():
    text, code = header()
    for name in CALLS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
    assert re.search(r"#define\s+RAU_XNORM_NONE\s+0\b", text)
    assert re.search(r"#define\s+RAU_XNORM_L2\s+1\b", text)
    assert re.search(r"#define\s+RAU_ABI_VERSION\s+5\b", text)
    assert (_lib.XNORM_NONE, _lib.XNORM_L2) == (0, 1)


def test_library_exports_and_bindings_cover_the_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name
        assert re.search(r"\bint %s\s*\(" % name, cdef), name
    for method in ("normalizeFeatures", "featNorm", "normFeats"):
        assert "function RAU:%s(" % method in lua, method
