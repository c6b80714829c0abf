"""Tied feature-map dropout, host side: the three places that declare rau_set_feat_dropout / rau_feat_dropout
(include/rau.h, bindings/rau.lua, rau_vqa_amd/_lib.py), the ABI version, and the mask shapes of the Python layer."""
import os
import re

from rau_vqa_amd import _lib
from rau_vqa_amd.model import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = ("int rau_set_feat_dropout(rau_ctx* ctx, int kind);", "int rau_feat_dropout(rau_ctx* ctx, int* kind);")


def _code(path):
    text = open(os.path.join(ROOT, *path)).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_header_declares_the_switch_and_keeps_the_abi_version():
    header = _code(("include", "rau.h"))
    for p in PROTOS:
        assert p in header, p
    assert "#define RAU_XDROP_PER_HOP 0" in header and "#define RAU_XDROP_TIED 1" in header
    assert "#define RAU_ABI_VERSION 5 " in header
    assert (_lib.XDROP_PER_HOP, _lib.XDROP_TIED) == (0, 1)


def test_lua_shim_declares_and_wraps_the_switch():
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    cdef = re.sub(r"\s+", " ", "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S)))
    for p in PROTOS:
        assert p in cdef, p
    assert "function RAU:tieFeatureDropout(on)" in lua and "C.rau_set_feat_dropout(self.h" in lua


def test_ctypes_table_binds_both_calls():
    import ctypes as C
    assert _lib._SIGS["rau_set_feat_dropout"] == (C.c_int, [C.c_void_p, C.c_int])
    res, args = _lib._SIGS["rau_feat_dropout"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1] is C.POINTER(C.c_int)
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rau_set_feat_dropout") and hasattr(lib, "rau_feat_dropout")
    # argument checks that need no device
    bound = _lib.lib()
    assert bound.rau_set_feat_dropout(None, 1) == -1 and b"null" in bound.rau_last_error()


def test_mask_shapes_of_the_tied_site():
    cfg = Config(B=6, T=5, E=8, Rq=16, D=24, S=49, M=40, H=3)
    per_hop, tied = cfg.mask_shapes(), cfg.mask_shapes(tied_x=True)
    assert per_hop["x"] == (3, 6, 24, 49) and tied["x"] == (6, 24, 49)
    assert {k: v for k, v in tied.items() if k != "x"} == {k: v for k, v in per_hop.items() if k != "x"}
    assert cfg.mask_shapes(4, tied_x=True)["x"] == (4, 24, 49)
    assert cfg.mask_shapes(4)["x"] == (3, 4, 24, 49)
