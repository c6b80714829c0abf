"""Element types of a batch's feature map (``rau_feat_type`` of include/rau.h), on the host.

A batch may be handed over as f32, IEEE fp16 or bf16.  numpy has fp16 (``np.float16``) but no bf16,
so bf16 maps travel as ``uint16`` bit patterns and must be named explicitly: a ``uint16`` array
without ``feat_type="bf16"`` is an error, never a guess.  Widening either 16-bit form to f32 is exact,
and the library's results for a 16-bit batch are bit-identical to those for the widened f32 batch.

The two OCP fp8 formats, ``e4m3`` (e4m3fn: bias 7, no infinities, S.1111.111 the NaN, largest finite 448)
and ``e5m2`` (bias 15, infinities and NaNs as in binary16, largest finite 57344), follow the same rules:
they travel as ``uint8`` bit patterns and must be named explicitly -- a ``uint8`` array without
``feat_type`` is an error, never a guess -- every code widens to f32 exactly, and results are
bit-identical to those for the widened f32 batch.  ``fp8_bits`` is the narrowing contract (round to
nearest even, saturating at the largest finite value), the one the device follows in ``bank_put``.
What fp8 storage does to VQA accuracy is not measured and not claimed: the contract is exactness with
respect to the stored values, and choosing a format is the user's decision (e4m3 has 3 significand bits
and range up to 448, e5m2 has 2 bits and range up to 57344).
Nothing here touches a device.
"""
from __future__ import annotations

import numpy as np

FEAT_TYPES = {"f32": 0, "f16": 1, "bf16": 2, "e4m3": 4, "e5m2": 5}   # name -> rau_feat_type (3 is reserved)
FEAT_NAMES = {v: k for k, v in FEAT_TYPES.items()}
_DTYPES = {"f32": np.float32, "f16": np.float16, "bf16": np.uint16, "e4m3": np.uint8, "e5m2": np.uint8}
# fp8 formats: (mantissa bits, exponent bias, largest finite value)
_FP8 = {"e4m3": (3, 7, 448.0), "e5m2": (2, 15, 57344.0)}


def dtype_of(feat_type: str):
    """numpy dtype of a map of `feat_type` (bf16: its uint16 bit patterns; fp8: its uint8 bit patterns)."""
    check_name(feat_type)
    return np.dtype(_DTYPES[feat_type])


def check_name(feat_type: str) -> str:
    if feat_type not in FEAT_TYPES:
        raise ValueError(f"feat_type {feat_type!r}: one of {sorted(FEAT_TYPES)}")
    return feat_type


def infer(feats, feat_type=None) -> str:
    """The feature type a batch array stands for: `feat_type` if given, else from its dtype
    (float16 -> "f16", other numbers -> "f32"; uint16 and uint8 are ambiguous and rejected)."""
    dt = np.asarray(feats).dtype
    if feat_type is not None:
        check_name(feat_type)
        if feat_type in _FP8 and dt != np.uint8:
            raise ValueError(f"feat_type {feat_type!r} takes uint8 bit patterns, not {dt} (see fp8_bits)")
        if feat_type not in _FP8 and dt == np.uint8:
            raise ValueError(f"uint8 arrays are fp8 bit patterns (feat_type 'e4m3' | 'e5m2'), not {feat_type!r}")
        if feat_type == "bf16" and dt != np.uint16:
            raise ValueError(f"feat_type 'bf16' takes uint16 bit patterns, not {dt}")
        if feat_type == "f16" and dt == np.uint16:
            raise ValueError("feat_type 'f16' takes float16 arrays (view uint16 bits as np.float16)")
        return feat_type
    if dt == np.uint16:
        raise ValueError("uint16 feature maps need an explicit feat_type='bf16'")
    if dt == np.uint8:
        raise ValueError("uint8 feature maps need an explicit feat_type='e4m3' or 'e5m2'")
    return "f16" if dt == np.float16 else "f32"


def as_feats(feats, feat_type=None):
    """-> (C-contiguous array in the element type, its name).  f32 and f16 arrays of another
    floating type are converted by numpy (round to nearest even); bf16 and fp8 must already be bits."""
    name = infer(feats, feat_type)
    return np.ascontiguousarray(feats, _DTYPES[name]), name


def bf16_bits(a) -> np.ndarray:
    """f32 values -> bf16 bit patterns, round to nearest even (finite inputs)."""
    x = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((x + (((x >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16)


def fp8_bits(a, feat_type: str) -> np.ndarray:
    """f32 values -> OCP fp8 codes (uint8) of `feat_type` "e4m3" | "e5m2": THE narrowing contract.

    Round to nearest even; every result beyond the largest finite value (448 / 57344) becomes that value
    with the input's sign, +-inf included (saturating); NaN becomes a NaN code; magnitudes at or below half
    the smallest subnormal become +-0; the sign is the input's sign bit.  With emin = 1 - bias:
    e = max(floor(log2 |x|), emin), q = 2^(e - mbits), r = min(rint(|x| / q) * q, largest finite)."""
    if feat_type not in _FP8:
        raise ValueError(f"fp8_bits: feat_type {feat_type!r}: 'e4m3' or 'e5m2'")
    mbits, bias, maxf = _FP8[feat_type]
    emin = 1 - bias
    x = np.ascontiguousarray(a, np.float32)
    sign = ((x.view(np.uint32) >> 24) & 0x80).astype(np.uint8)
    nan = np.isnan(x)
    mag = np.abs(np.where(nan, np.float32(0), x).astype(np.float64))
    mag = np.minimum(mag, 2.0 * maxf)                    # inf and huge values: anything that saturates
    _, ex = np.frexp(mag)                                # mag = f * 2^ex, f in [0.5, 1): floor(log2) = ex - 1
    e = np.maximum(ex.astype(np.int64) - 1, emin)        # (mag == 0: ex = 0, e = emin)
    r = np.minimum(np.ldexp(np.rint(np.ldexp(mag, mbits - e)), e - mbits), maxf)   # rint: to nearest even
    # r is a value of the format: encode it (rounding may have carried it into the next exponent)
    _, ex = np.frexp(r)
    e = np.maximum(ex.astype(np.int64) - 1, emin)
    m = np.ldexp(r, mbits - e).astype(np.int64)          # in [0, 2^(mbits+1)); below 2^mbits: subnormal or zero
    code = np.where(m < 2 ** mbits, m, ((e + bias) << mbits) | (m - 2 ** mbits)).astype(np.uint8)
    return np.where(nan, np.uint8(0x7F), code) | sign


def widen(a, feat_type: str) -> np.ndarray:
    """A map of `feat_type` as the f32 values it stands for (exact)."""
    check_name(feat_type)
    a = np.asarray(a)
    if feat_type == "e5m2":                              # the upper byte of a binary16
        return (a.astype(np.uint16) << 8).view(np.float16).astype(np.float32)
    if feat_type == "e4m3":
        c = a.astype(np.uint32)
        e, m = (c >> 3) & 0xF, c & 7
        v = np.where(e == 0, np.ldexp(m.astype(np.float32), -9),
                     np.ldexp((8 + m).astype(np.float32), e.astype(np.int32) - 10)).astype(np.float32)
        v = np.where((c & 0x7F) == 0x7F, np.float32(np.nan), v)
        return (v.view(np.uint32) | ((c & 0x80) << 24)).view(np.float32)
    if feat_type == "bf16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def store(dst: np.ndarray, src, feat_type=None) -> None:
    """dst[...] = src converted to dst's element type (float32, float16, bf16 bits as uint16, or fp8 codes as
    uint8).  A uint8 `dst` does not say which fp8 format it holds: name it with `feat_type` unless `src` is
    uint8 codes already."""
    if dst.dtype == np.uint8:
        src = np.asarray(src)
        if src.dtype != np.uint8:
            if feat_type not in _FP8:
                raise ValueError("store into uint8 (fp8 codes) needs feat_type='e4m3' or 'e5m2'")
            src = fp8_bits(src.astype(np.float32), feat_type).reshape(dst.shape)
        dst[...] = src
    elif dst.dtype == np.uint16:
        src = np.asarray(src)
        dst[...] = src if src.dtype == np.uint16 else bf16_bits(src.astype(np.float32)).reshape(dst.shape)
    else:
        dst[...] = src


def check_counts(counts, S: int) -> np.ndarray:
    """Region counts of a packed batch as a 1-D int32 array: every entry in 1..S."""
    n = np.asarray(counts)
    if n.ndim != 1 or n.size < 1 or not np.issubdtype(n.dtype, np.integer):
        raise ValueError(f"counts: a 1-D integer array with at least one entry, not {n.dtype}{n.shape}")
    if n.min() < 1 or n.max() > S:
        raise ValueError(f"counts must lie in 1..S={S}: got {int(n.min())}..{int(n.max())}")
    return np.ascontiguousarray(n, np.int32)


def unpack_regions(rows, counts, S: int) -> np.ndarray:
    """Packed region rows -> dense maps: THE contract of the packed entry points.

    rows [sum(counts), D] in any element type (float32, float16, uint16 or uint8 codes), counts [N] with
    1 <= counts[i] <= S.  -> dense [N, D, S] of the same dtype with dense[i, :, s] = rows[off[i] + s, :] for
    s < counts[i], off the exclusive prefix sum; every other element has all bits zero (+0 in every type)."""
    n = check_counts(counts, S)
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[0] != int(n.sum()):
        raise ValueError(f"rows {rows.shape}: expected [sum(counts)={int(n.sum())}, D]")
    dense = np.zeros((n.size, rows.shape[1], S), rows.dtype)
    off = 0
    for i, c in enumerate(n):
        dense[i, :, :c] = rows[off:off + c].T
        off += int(c)
    return dense


def l2_normalize(x, eps=1e-12) -> np.ndarray:
    """Per-position L2 normalisation of maps [..., D, S] over the channel axis, the statement of
    ``rau_set_feat_norm``: ``x / max(sqrt(sum_d x^2), eps)``, computed in float64 and rounded to float32 once."""
    x = np.asarray(x, np.float64)
    nrm = np.sqrt(np.sum(x * x, axis=-2, keepdims=True))
    return (x / np.maximum(nrm, float(eps))).astype(np.float32)


def l2_normalize_grad(x, g, eps=1e-12) -> np.ndarray:
    """Gradient at ``x`` of ``l2_normalize(x, eps)`` for the gradient ``g`` at its output (same shape): with
    ``xn = x / max(nrm, eps)`` and ``c = sum_d g xn``, ``(g - xn c) / nrm`` where ``nrm >= eps`` and ``g / eps``
    where ``nrm < eps`` (the forward is linear there).  float64, rounded to float32 once."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    nrm = np.sqrt(np.sum(x * x, axis=-2, keepdims=True))
    r = 1.0 / np.maximum(nrm, float(eps))
    xn = x * r
    c = np.sum(g * xn, axis=-2, keepdims=True)
    return (r * (g - np.where(nrm >= float(eps), xn * c, 0.0))).astype(np.float32)
