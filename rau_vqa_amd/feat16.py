"""Element types of a batch's feature map (``rau_feat_type`` of include/rau.h), on the host.

A batch may be handed over as f32, IEEE fp16 or bf16.  numpy has fp16 (``np.float16``) but no bf16,
so bf16 maps travel as ``uint16`` bit patterns and must be named explicitly: a ``uint16`` array
without ``feat_type="bf16"`` is an error, never a guess.  Widening either 16-bit form to f32 is exact,
and the library's results for a 16-bit batch are bit-identical to those for the widened f32 batch.
Nothing here touches a device.
"""
from __future__ import annotations

import numpy as np

FEAT_TYPES = {"f32": 0, "f16": 1, "bf16": 2}          # name -> rau_feat_type
FEAT_NAMES = {v: k for k, v in FEAT_TYPES.items()}
_DTYPES = {"f32": np.float32, "f16": np.float16, "bf16": np.uint16}


def dtype_of(feat_type: str):
    """numpy dtype of a map of `feat_type` (bf16: its uint16 bit patterns)."""
    check_name(feat_type)
    return np.dtype(_DTYPES[feat_type])


def check_name(feat_type: str) -> str:
    if feat_type not in FEAT_TYPES:
        raise ValueError(f"feat_type {feat_type!r}: one of {sorted(FEAT_TYPES)}")
    return feat_type


def infer(feats, feat_type=None) -> str:
    """The feature type a batch array stands for: `feat_type` if given, else from its dtype
    (float16 -> "f16", other numbers -> "f32"; uint16 is ambiguous and rejected)."""
    dt = np.asarray(feats).dtype
    if feat_type is not None:
        check_name(feat_type)
        if feat_type == "bf16" and dt != np.uint16:
            raise ValueError(f"feat_type 'bf16' takes uint16 bit patterns, not {dt}")
        if feat_type == "f16" and dt == np.uint16:
            raise ValueError("feat_type 'f16' takes float16 arrays (view uint16 bits as np.float16)")
        return feat_type
    if dt == np.uint16:
        raise ValueError("uint16 feature maps need an explicit feat_type='bf16'")
    return "f16" if dt == np.float16 else "f32"


def as_feats(feats, feat_type=None):
    """-> (C-contiguous array in the element type, its name).  f32 and f16 arrays of another
    floating type are converted by numpy (round to nearest even); bf16 must already be bits."""
    name = infer(feats, feat_type)
    return np.ascontiguousarray(feats, _DTYPES[name]), name


def bf16_bits(a) -> np.ndarray:
    """f32 values -> bf16 bit patterns, round to nearest even (finite inputs)."""
    x = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((x + (((x >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16)


def widen(a, feat_type: str) -> np.ndarray:
    """A map of `feat_type` as the f32 values it stands for (exact)."""
    check_name(feat_type)
    a = np.asarray(a)
    if feat_type == "bf16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def store(dst: np.ndarray, src) -> None:
    """dst[...] = src converted to dst's element type (float32, float16 or bf16 bits as uint16)."""
    if dst.dtype == np.uint16:
        src = np.asarray(src)
        dst[...] = src if src.dtype == np.uint16 else bf16_bits(src.astype(np.float32)).reshape(dst.shape)
    else:
        dst[...] = src
