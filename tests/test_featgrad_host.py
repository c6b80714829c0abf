"""Feature-map gradient (rau_set_feat_grad, rau_feat_grad_dev, rau_get_feat_grad, rau_set_batch_dev) on the host
side: the three places that declare the calls agree, and the numpy statement of the masked hop sum
(tests/featgrad_ref.py: masked_hop_sum, the arithmetic of xgrad.hip's accumulate pass) is the gradient of the masked
1x1 convolution -- including a pitched map, whose mask is indexed over the LOGICAL [.., S] tensor."""
import ctypes as C
import os
import re

import numpy as np
import torch

from rau_vqa_amd import _lib
from tests import featgrad_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "rau_set_feat_grad": "int rau_set_feat_grad(rau_ctx* ctx, int on);",
    "rau_feat_grad": "int rau_feat_grad(rau_ctx* ctx, int* on);",
    "rau_feat_grad_dev": "int rau_feat_grad_dev(rau_ctx* ctx, const float** dX, int32_t* pitch);",
    "rau_get_feat_grad": "int rau_get_feat_grad(rau_ctx* ctx, float* host",
    "rau_set_batch_dev": "int rau_set_batch_dev(rau_ctx* ctx, const float* feats_dev",
}


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_has_the_prototypes_at_abi_5():
    header = read("include", "rau.h")
    assert re.search(r"#define RAU_ABI_VERSION 5\b", header)
    for name, proto in PROTOS.items():
        assert proto in header, name
    # the contract the callers rely on is stated where the calls are declared
    for phrase in ("OVERWRITTEN", "rau_zero_grads does not touch it", "image-table or bank batch", "x[image_of]"):
        assert phrase in header, phrase


def test_lua_and_ctypes_agree_with_the_header():
    lua = read("bindings", "rau.lua")
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    header = re.sub(r"/\*.*?\*/", "", read("include", "rau.h"), flags=re.S)
    for name in PROTOS:
        assert re.search(r"\bint %s\s*\(" % name, cdef), name
        # same number of parameters in the header, the cdef and the ctypes table
        count = lambda text: len(re.search(r"\bint %s\s*\((.*?)\);" % name, text, flags=re.S).group(1).split(","))
        assert count(header) == count(cdef) == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is C.c_int
    for fn, call in (("wantFeatureGrad", "rau_set_feat_grad"), ("featureGrad", "rau_feat_grad_dev"),
                     ("setBatchDev", "rau_set_batch_dev")):
        assert "function RAU:%s(" % fn in lua and "C.%s(self.h" % call in lua, fn
    assert _lib._SIGS["rau_feat_grad_dev"][1] == [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    model = read("rau_vqa_amd", "model.py")
    for fn in ("want_feature_grad", "feature_grad_wanted", "feature_grad", "feature_grad_tensor", "set_batch_dev"):
        assert "def %s(" % fn in model, fn


def test_the_library_exports_the_calls_and_checks_null():
    lib = _lib.lib()
    assert lib.rau_abi_version() == 5
    assert lib.rau_set_feat_grad(None, 1) == -1 and b"null" in lib.rau_last_error()
    assert lib.rau_feat_grad(None, None) == -1
    assert lib.rau_feat_grad_dev(None, None, None) == -1
    assert lib.rau_get_feat_grad(None, None) == -1
    assert lib.rau_set_batch_dev(None, None, None, None, None) == -1


def pack_bits(keep):
    """The site's bit-packed form: bit e & 31 of word e >> 5 for flat element e of the logical tensor."""
    flat = np.asarray(keep, np.uint8).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, np.uint32)
    for e in np.nonzero(flat)[0]:
        words[e >> 5] |= np.uint32(1) << np.uint32(e & 31)
    return words


def kernel_index_keep(words, hop, n, D, S, Sp):
    """The keep bits as the accumulate pass reads them for a pitched buffer [n*D rows][Sp]: row r, position s < S is
    element e0 + r * S + s of the site, e0 = hop * n * D * S; pad positions have no bit (0)."""
    out = np.zeros((n * D, Sp), np.uint8)
    e0 = hop * n * D * S
    for r in range(n * D):
        for s in range(S):
            e = e0 + r * S + s
            out[r, s] = (int(words[e >> 5]) >> (e & 31)) & 1
    return out.reshape(n, D, Sp)


def check_masked_hop_sum(S):
    d = dict(util.EDGE, S=S, H=3)
    n, D, M, H = d["B"], d["D"], d["M"], d["H"]
    Sp = (S + 3) // 4 * 4
    p = 0.5
    rng = np.random.default_rng(11)
    W = rng.normal(size=(M, D))
    dZ = rng.normal(size=(H, n, M, S))
    keep = (rng.random(size=(H, n, D, S)) >= p).astype(np.uint8)
    # fp64 autograd: L = sum_h <dZ_h, W (x * keep_h / (1 - p))>  =>  dL/dx = sum_h keep_h / (1 - p) * W^T dZ_h
    x = torch.zeros(n, D, S, dtype=torch.float64, requires_grad=True)
    loss = sum((torch.as_tensor(dZ[h]) * torch.einsum("md,bds->bms", torch.as_tensor(W),
                                                      x * torch.as_tensor(keep[h]) / (1 - p))).sum()
               for h in range(H))
    loss.backward()
    # the per-hop products at pitch Sp, with junk in the pad columns: they must not reach the result
    G = np.full((H, n, D, Sp), 7.0, np.float32)
    G[..., :S] = np.einsum("md,hbms->hbds", W, dZ)
    # the bits travel packed over the LOGICAL tensor and come back through the kernel's index
    words = pack_bits(keep)
    got_keep = np.stack([kernel_index_keep(words, h, n, D, S, Sp) for h in range(H)])
    assert np.array_equal(got_keep[..., :S], keep) and not got_keep[..., S:].any()
    for order in (None, [2, 0, 1]):
        dX = featgrad_ref.masked_hop_sum(G, got_keep[..., :S], p, S, Sp, order)
        assert dX.dtype == np.float32 and dX.shape == (n, D, Sp)
        assert util.rel_err(dX[..., :S], x.grad.numpy()) < 1e-6
        assert not dX[..., S:].any()
    # no mask (evaluate mode): scale 1
    x0 = featgrad_ref.masked_hop_sum(G, None, p, S, Sp)
    assert util.rel_err(x0[..., :S], np.einsum("md,hbms->bds", W, dZ)) < 1e-6
    # a zero product under a kept bit is a zero TERM, not a dropped one: the bits are never inferred from values
    G0 = G.copy()
    G0[0] = 0
    assert np.array_equal(featgrad_ref.masked_hop_sum(G0, got_keep[..., :S], p, S, Sp),
                          featgrad_ref.masked_hop_sum(G[1:], got_keep[1:, ..., :S], p, S, Sp)[...] + np.float32(0))


def test_masked_hop_sum_on_the_edge_shape():
    check_masked_hop_sum(util.EDGE["S"])


def test_masked_hop_sum_pitched_mask_indexing():
    check_masked_hop_sum(5)      # pitch 8: rows of the mask are 5 bits long, rows of the data 8 floats
    check_masked_hop_sum(49)     # pitch 52: words of the mask straddle rows
