"""16-bit feature maps on the host (no device): feature-type inference and rejection
(rau_vqa_amd/feat16.py), Torch7 HalfTensor files (t7.py) and the loader filling fp16 / bf16
destinations (loader.py).  The device half is tests/test_gpu_feat16.py."""
import struct

import numpy as np
import pytest

from rau_vqa_amd import feat16, loader, t7
from tests.test_loader import D, H, T, W, _FakeRau, dataset  # noqa: F401  (fixture)


def test_feat_type_inference_and_rejection():
    f32 = np.ones((2, 3), np.float32)
    assert feat16.infer(f32) == "f32"
    assert feat16.infer(np.ones(3, np.float64)) == "f32"
    assert feat16.infer(f32.astype(np.float16)) == "f16"
    bits = np.zeros(3, np.uint16)
    with pytest.raises(ValueError, match="bf16"):
        feat16.infer(bits)                                  # uint16 alone is ambiguous
    assert feat16.infer(bits, "bf16") == "bf16"
    with pytest.raises(ValueError):
        feat16.infer(f32, "bf16")                           # bf16 comes as bit patterns only
    with pytest.raises(ValueError):
        feat16.infer(bits, "f16")
    with pytest.raises(ValueError, match="feat_type"):
        feat16.infer(f32, "fp8")
    a, name = feat16.as_feats(np.full(4, 1.0 / 3.0), "f16")
    assert name == "f16" and a.dtype == np.float16 and a.flags.c_contiguous
    assert feat16.dtype_of("bf16") == np.uint16 and feat16.dtype_of("f16") == np.float16


def test_widening_is_exact_and_bf16_rounding_is_nearest_even():
    allf16 = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16)
    fin = np.isfinite(allf16)
    w = feat16.widen(allf16[fin], "f16")
    assert w.dtype == np.float32
    np.testing.assert_array_equal(w.astype(np.float16).view(np.uint16), allf16[fin].view(np.uint16))
    sub = allf16[fin][(allf16[fin].view(np.uint16) & 0x7C00) == 0]   # +-0 and the subnormals
    np.testing.assert_array_equal(feat16.widen(sub, "f16"), sub.astype(np.float64).astype(np.float32))
    b = np.array([0x3F80, 0x8001, 0x0001, 0x7F7F, 0xC2F7], np.uint16)
    wb = feat16.widen(b, "bf16")
    np.testing.assert_array_equal(wb.view(np.uint32) >> 16, b)
    np.testing.assert_array_equal(wb.view(np.uint32) & 0xFFFF, 0)
    np.testing.assert_array_equal(feat16.bf16_bits(wb), b)
    x = np.array([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8 + 2 ** -20, -(1.0 + 2 ** -8)], np.float32)
    np.testing.assert_array_equal(feat16.bf16_bits(x), [0x3F80, 0x3F82, 0x3F81, 0xBF80])


def test_t7_half_tensor_round_trip_and_reading(tmp_path):
    a = (np.arange(24, dtype=np.float32).reshape(2, 3, 4) / 7).astype(np.float16)
    a.view(np.uint16)[0, 0, :2] = [0x0001, 0x83FF]          # two subnormals survive the file
    t7.save(tmp_path / "h.t7", a)
    back = t7.load(tmp_path / "h.t7")
    assert back.type_name == "torch.HalfTensor" and back.array.dtype == np.float16
    np.testing.assert_array_equal(back.array.view(np.uint16), a.view(np.uint16))
    # reader on a hand-assembled HalfTensor (independent of the writer)
    i32, i64 = (lambda v: struct.pack("<i", v)), (lambda v: struct.pack("<q", v))
    s = lambda txt: i32(len(txt)) + txt.encode()
    vals = np.array([1.5, -2.0, 65504.0], np.float16)
    raw = (i32(4) + i32(1) + s("V 1") + s("torch.HalfTensor") + i32(1) + i64(3) + i64(1) + i64(1)
           + i32(4) + i32(2) + s("V 1") + s("torch.HalfStorage") + i64(3) + vals.astype("<f2").tobytes())
    np.testing.assert_array_equal(t7.loads(raw).array, vals)
    # load_feature: f32 by default (the existing contract), float16 kept on request
    f = a.reshape(2, 3, 4)
    assert t7.load_feature(tmp_path / "h.t7", 2, 3, 4).dtype == np.float32
    kept = t7.load_feature(tmp_path / "h.t7", 2, 3, 4, keep_half=True)
    assert kept.dtype == np.float16 and kept.shape == (2, 12)
    np.testing.assert_array_equal(kept.view(np.uint16), f.reshape(2, 12).view(np.uint16))


def test_loader_fills_16bit_destinations(dataset, tmp_path):  # noqa: F811
    root, fdir, q, lens, feats = dataset
    B = 4
    ref = loader.load_data(str(root), batch_size=B).train_data
    v16 = loader.load_data(str(root), batch_size=B, feat_type="f16").train_data
    vb = loader.load_data(str(root), batch_size=B, feat_type="bf16").train_data
    for _ in range(3):
        f32 = ref.next_batch_feat(fdir, D, W, H)[0]
        f16 = v16.next_batch_feat(fdir, D, W, H)[0]
        fb = vb.next_batch_feat(fdir, D, W, H)[0]
        assert f16.dtype == np.float16 and fb.dtype == np.uint16 and f16.shape == f32.shape
        np.testing.assert_array_equal(f16, f32.astype(np.float16))      # f32 files rounded on assignment
        np.testing.assert_array_equal(fb, feat16.bf16_bits(f32))
    # HalfTensor files go into an fp16 destination as they are
    hdir = tmp_path / "half"
    hdir.mkdir()
    maps = [np.random.default_rng(i).standard_normal((D, W, H)).astype(np.float16) for i in range(2)]
    paths = []
    for i, m in enumerate(maps):
        paths.append(str(hdir / f"m{i}.t7"))
        t7.save(paths[-1], m)
    out = np.full((2, D, W * H), np.nan, np.float16)
    got = loader.DataClass._load_feats(paths, D, W, H, out)
    assert np.shares_memory(got, out)
    for i, m in enumerate(maps):
        np.testing.assert_array_equal(out[i].reshape(D, W, H).view(np.uint16), m.view(np.uint16))


class _FakeRau16(_FakeRau):
    """_FakeRau with typed slots: records the feat_type of each call."""

    def __init__(self, B, ft):
        super().__init__(B)
        for s in self.slots:
            s["feats"] = np.zeros(s["feats"].shape, feat16.dtype_of(ft))
        self.types = []

    def batch_slot(self, s, feat_type="f32"):
        self.types.append(feat_type)
        return self.slots[s]

    def set_batch_async(self, s, has_labels=True, feat_type="f32"):
        self.types.append(feat_type)
        super().set_batch_async(s, has_labels)


@pytest.mark.parametrize("ft", ["f16", "bf16"])
def test_slot_feeder_with_16bit_staging(dataset, ft):  # noqa: F811
    root, fdir, q, lens, feats = dataset
    B = 4
    ref = loader.load_data(str(root), batch_size=B).train_data
    v = loader.load_data(str(root), batch_size=B)
    rau = _FakeRau16(B, ft)
    feeder = loader.SlotFeeder(rau, v.train_data, fdir, D, W, H, feat_type=ft)
    for it in range(7):
        f = ref.next_batch_feat(fdir, D, W, H)[0].reshape(B, D, -1)
        want = f.astype(np.float16) if ft == "f16" else feat16.bf16_bits(f)
        np.testing.assert_array_equal(rau.current["feats"], want)
        if it < 6:
            feeder.next()
    assert set(rau.types) == {ft}
