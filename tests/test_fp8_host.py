"""fp8 feature maps (OCP e4m3fn / e5m2) on the host, no device: the exact widening of all 256 codes, the
narrowing contract ``feat16.fp8_bits`` (round to nearest even, saturating, include/rau.h), feature-type
inference and rejection, and the loader filling fp8 destinations.  The device half is
tests/test_gpu_fp8.py."""
import numpy as np
import pytest

from rau_vqa_amd import feat16, loader
from tests.test_feat16 import _FakeRau16
from tests.test_loader import D, H, W, dataset  # noqa: F401  (fixture)

# name -> (mantissa bits, exponent bias, largest finite value, torch dtype name)
FORMATS = {"e4m3": (3, 7, 448.0, "float8_e4m3fn"), "e5m2": (2, 15, 57344.0, "float8_e5m2")}
CODES = np.arange(256, dtype=np.uint8)


def torch_dtype(ft):
    try:
        import torch
    except Exception:
        return None, None
    return torch, getattr(torch, FORMATS[ft][3], None)


def table(ft):
    """The 256 values of the format from its field definitions (f64; NaN and inf where the format has them)."""
    mbits, bias, _, _ = FORMATS[ft]
    out = np.empty(256, np.float64)
    for c in range(256):
        s = -1.0 if c & 0x80 else 1.0
        e, m = (c & 0x7F) >> mbits, c & ((1 << mbits) - 1)
        emax = (1 << (7 - mbits)) - 1
        if ft == "e4m3" and (c & 0x7F) == 0x7F:
            v = np.nan
        elif ft == "e5m2" and e == emax:
            v = np.inf if m == 0 else np.nan
        elif e == 0:
            v = m * 2.0 ** (1 - bias - mbits)                      # +-0 and subnormals
        else:
            v = (1 + m / (1 << mbits)) * 2.0 ** (e - bias)
        out[c] = s * v
    return out


@pytest.mark.parametrize("ft", sorted(FORMATS))
def test_widening_of_all_256_codes_is_exact(ft):
    want = table(ft)
    w = feat16.widen(CODES, ft)
    assert w.dtype == np.float32 and w.shape == (256,)
    fin = np.isfinite(want)
    assert fin.sum() == (254 if ft == "e4m3" else 248)
    np.testing.assert_array_equal(w[fin].astype(np.float64), want[fin])
    np.testing.assert_array_equal(np.signbit(w), CODES >= 128)           # -0 keeps its sign, NaNs too
    np.testing.assert_array_equal(np.isnan(w), np.isnan(want))
    np.testing.assert_array_equal(w[np.isinf(want)], want[np.isinf(want)].astype(np.float32))
    assert np.all(np.abs(w[fin & (want != 0)]) >= 2.0 ** -16)            # subnormal codes are normal f32 numbers
    assert np.max(np.abs(w[fin])) == FORMATS[ft][2]
    # every finite code round-trips through the narrowing contract (-0 included)
    np.testing.assert_array_equal(feat16.fp8_bits(w[fin], ft), CODES[fin])
    torch, dt = torch_dtype(ft)
    if dt is not None:                                                   # cross-check only where torch has the type
        tw = torch.from_numpy(CODES.copy()).view(dt).to(torch.float32).numpy()
        np.testing.assert_array_equal(w[fin].view(np.uint32), tw[fin].view(np.uint32))


def values_and_codes(ft):
    """(f32 inputs, expected codes) of the narrowing cases; NaN inputs carry the expected code 0x7F and are
    compared by isnan.  Shared with the device test of rau_bank_put."""
    mbits, bias, maxf, _ = FORMATS[ft]
    emin = 1 - bias
    one = 1 << mbits                                                   # code distance of one binade
    xs, cs = [], []

    def add(x, c):
        xs.extend([x, -x])
        cs.extend([c, c | 0x80])
    # exact ties at several exponents, both parities: halfway between neighbouring codes c and c + 1
    for e in (emin, emin + 1, -1, 0, 1, 5):
        for m in range(one):
            c = ((e + bias) << mbits) | m
            lo = (1 + m / one) * 2.0 ** e
            ulp = 2.0 ** (e - mbits)
            add(lo + ulp / 2, c + (c & 1))                             # tie: to the even code
            add(np.nextafter(np.float32(lo + ulp / 2), np.float32(np.inf)), c + 1)
            add(np.nextafter(np.float32(lo + ulp / 2), np.float32(0)), c)
    # the subnormal range: units of u = 2^(emin - mbits)
    u = 2.0 ** (emin - mbits)
    for m in range(one):
        add(m * u, m)
        add((m + 0.5) * u, m + (m & 1))                                # m = 0: half the smallest subnormal -> 0
        add((m + 0.75) * u, m + 1)
        add((m + 0.25) * u, m)
    add(np.nextafter(np.float32(u / 2), np.float32(1)), 1)
    add(u / 4, 0)
    # around the largest finite value
    cmax = 0x7E if ft == "e4m3" else 0x7B
    top = 2.0 ** (np.floor(np.log2(maxf)) - mbits - 1)                 # half an ulp of the last binade
    for x in (maxf, maxf - top, np.nextafter(np.float32(maxf - top), np.float32(0)),
              np.nextafter(np.float32(maxf), np.float32(np.inf)), maxf + top,
              np.nextafter(np.float32(maxf + top), np.float32(np.inf)), maxf + 2 * top, 1e10, np.inf):
        want = cmax
        if x < maxf - top:
            want = cmax - 1
        elif x == maxf - top:                                          # a tie below the maximum
            want = cmax - 1 if (cmax - 1) % 2 == 0 else cmax
        add(x, want)
    # f32 subnormals and zeros
    for x in (0.0, 1e-45, 1e-39, 2.0 ** -126):
        add(x, 0)
    xs += [np.nan, -np.nan]
    cs += [0x7F, 0x7F]
    return np.array(xs, np.float32), np.array(cs, np.uint8)


@pytest.mark.parametrize("ft", sorted(FORMATS))
def test_narrowing_contract_cases(ft):
    x, want = values_and_codes(ft)
    got = feat16.fp8_bits(x, ft)
    assert got.dtype == np.uint8
    nan = np.isnan(x)
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert np.all(np.isnan(feat16.widen(got[nan], ft)))
    # the values named in the contract
    def bits(*v):
        return list(feat16.fp8_bits(np.array(v, np.float32), ft))
    if ft == "e4m3":
        assert bits(448, 464, 465, 463, 480, 1e10, np.inf, -np.inf) == [0x7E] * 7 + [0xFE]
        assert bits(432, 431.9, 2.0 ** -10, 2.0 ** -10 * 1.01, -0.0) == [0x7E, 0x7D, 0, 1, 0x80]
    else:
        assert bits(57344, 61440, 61441, 65536, 1e10, np.inf, -np.inf) == [0x7B] * 6 + [0xFB]
        assert bits(53248, 53249, 2.0 ** -17, 2.0 ** -17 * 1.01, -0.0) == [0x7A, 0x7B, 0, 1, 0x80]
    with pytest.raises(ValueError):
        feat16.fp8_bits(x, "f16")


@pytest.mark.parametrize("ft", sorted(FORMATS))
def test_narrowing_equals_the_numpy_statement_and_torch(ft):
    """The contract as include/rau.h words it, evaluated literally in f64, and torch's CPU cast where
    |x| <= the largest finite value (torch does not saturate)."""
    mbits, bias, maxf, _ = FORMATS[ft]
    emin = 1 - bias
    rng = np.random.default_rng(7)
    n = 200_000
    x = (rng.standard_normal(n) * np.exp(rng.uniform(np.log(1e-3), np.log(300.0), n))).astype(np.float32)
    x = np.concatenate([x, (x * 2.0 ** -12).astype(np.float32), (x * 200).astype(np.float32)])
    a = np.abs(x.astype(np.float64))
    e = np.maximum(np.floor(np.log2(np.maximum(a, 1e-300))), emin)
    q = 2.0 ** (e - mbits)
    r = np.minimum(np.rint(a / q) * q, maxf)
    got = feat16.fp8_bits(x, ft)
    np.testing.assert_array_equal(np.abs(feat16.widen(got, ft)).astype(np.float64), r)
    np.testing.assert_array_equal(got >> 7, np.signbit(x).astype(np.uint8))
    torch, dt = torch_dtype(ft)
    if dt is not None:
        ok = np.abs(x) <= maxf
        tb = torch.from_numpy(x[ok]).to(dt).view(torch.uint8).numpy()
        np.testing.assert_array_equal(got[ok], tb)


def test_feat_type_inference_and_rejection():
    codes = np.zeros((2, 3), np.uint8)
    with pytest.raises(ValueError, match="e4m3"):
        feat16.infer(codes)                                 # uint8 alone is ambiguous: never a guess
    with pytest.raises(ValueError):
        feat16.as_feats(codes)
    for ft in FORMATS:
        assert feat16.infer(codes, ft) == ft
        a, name = feat16.as_feats(codes[:, ::2], ft)
        assert name == ft and a.dtype == np.uint8 and a.flags.c_contiguous
        assert feat16.dtype_of(ft) == np.uint8
        for wrong in (np.ones(3, np.float32), np.ones(3, np.float16), np.zeros(3, np.uint16), np.zeros(3, np.int8)):
            with pytest.raises(ValueError):
                feat16.infer(wrong, ft)                     # fp8 comes as uint8 bit patterns only
    for other in ("f32", "f16", "bf16"):
        with pytest.raises(ValueError):
            feat16.infer(codes, other)
    assert feat16.FEAT_TYPES["e4m3"] == 4 and feat16.FEAT_TYPES["e5m2"] == 5
    assert 3 not in feat16.FEAT_NAMES                       # reserved
    # store: codes are copied, numbers are narrowed and need the format's name
    dst = np.zeros(4, np.uint8)
    feat16.store(dst, np.array([1, 2, 3, 4], np.uint8))
    np.testing.assert_array_equal(dst, [1, 2, 3, 4])
    feat16.store(dst, np.array([1.0, -2.0, 0.5, 1e9], np.float32), "e4m3")
    np.testing.assert_array_equal(dst, [0x38, 0xC0, 0x30, 0x7E])
    feat16.store(dst, np.array([1.0, -2.0, 0.5, np.inf], np.float16), "e5m2")   # inf saturates
    np.testing.assert_array_equal(dst, [0x3C, 0xC0, 0x38, 0x7B])
    with pytest.raises(ValueError):
        feat16.store(dst, np.ones(4, np.float32))


@pytest.mark.parametrize("ft", sorted(FORMATS))
def test_loader_yields_fp8_bits_of_the_f32_loader(dataset, ft):  # noqa: F811
    root, fdir, q, lens, feats = dataset
    B = 4
    ref = loader.load_data(str(root), batch_size=B).train_data
    v8 = loader.load_data(str(root), batch_size=B, feat_type=ft).train_data
    for _ in range(3):
        f32 = ref.next_batch_feat(fdir, D, W, H)[0]
        f8 = v8.next_batch_feat(fdir, D, W, H)[0]
        assert f8.dtype == np.uint8 and f8.shape == f32.shape
        np.testing.assert_array_equal(f8, feat16.fp8_bits(f32, ft))
    t32, io32 = (lambda b: (b[0], b[5]))(ref.next_batch_feat(fdir, D, W, H, unique=True))
    t8, io8 = (lambda b: (b[0], b[5]))(v8.next_batch_feat(fdir, D, W, H, unique=True))
    np.testing.assert_array_equal(t8, feat16.fp8_bits(t32, ft))
    np.testing.assert_array_equal(io8, io32)


@pytest.mark.parametrize("ft", sorted(FORMATS))
def test_slot_feeder_with_fp8_staging(dataset, ft):  # noqa: F811
    root, fdir, q, lens, feats = dataset
    B = 4
    ref = loader.load_data(str(root), batch_size=B).train_data
    v = loader.load_data(str(root), batch_size=B)
    rau = _FakeRau16(B, ft)
    assert rau.slots[0]["feats"].dtype == np.uint8
    feeder = loader.SlotFeeder(rau, v.train_data, fdir, D, W, H, feat_type=ft)
    for it in range(7):
        f = ref.next_batch_feat(fdir, D, W, H)[0].reshape(B, D, -1)
        np.testing.assert_array_equal(rau.current["feats"], feat16.fp8_bits(f, ft))
        if it < 6:
            feeder.next()
    assert set(rau.types) == {ft}                           # batch_slot and set_batch_async both got the type


class _FakeBankRau:
    """Records what fill_bank puts: f32 maps go up as f32 for the device to narrow."""

    def __init__(self, cap, ft):
        self.info, self.puts = {"capacity": cap, "feat_type": ft, "rows_filled": 0}, []

    def bank_info(self):
        return dict(self.info)

    def bank_put(self, first, feats, feat_type=None):
        self.puts.append((first, np.asarray(feats).dtype, feat_type))


def test_fill_bank_lets_the_device_narrow(dataset):  # noqa: F811
    root, fdir, q, lens, feats = dataset
    data = loader.load_data(str(root), batch_size=4).train_data
    files, _ = data.bank_rows(fdir)
    rau = _FakeBankRau(len(files), "e4m3")
    assert data.fill_bank(rau, fdir, D, W, H, chunk=3) == len(files)
    assert rau.puts and all(dt == np.float32 and ft is None for _, dt, ft in rau.puts)
