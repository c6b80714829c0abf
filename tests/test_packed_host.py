"""Packed region features on the host side: the header, the numpy contract (feat16.unpack_regions), the loader's
packed batches against its dense ones, and the GPU tests' table of shapes held to the unpack kernel's tile constants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rau_vqa_amd import feat16, loader, t7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rau_set_batch_packed", "rau_set_batch_async_packed", "rau_bank_put_packed")


# ---------------------------------------------------------------- header and library
def test_header_declares_the_three_calls_and_keeps_abi_5():
    from rau_vqa_amd import _lib
    text = open(os.path.join(ROOT, "include", "rau.h")).read()
    assert re.search(r"#define\s+RAU_ABI_VERSION\s+5\b", text)
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*rau_ctx\s*\*", text), name
        assert name in _lib._SIGS
    lib = C.CDLL(_lib.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
    lib.rau_abi_version.restype = C.c_int
    assert lib.rau_abi_version() == 5
    # argument counts of the prototypes the loader binds, against the header's
    for name in CALLS:
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text).group(1)
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S)
        assert len(args.split(",")) == len(_lib._SIGS[name][1]), name


# ---------------------------------------------------------------- the contract
def plain_loop(rows, counts, S):
    out = np.zeros((len(counts), rows.shape[1], S), rows.dtype)
    r = 0
    for i, c in enumerate(counts):
        for s in range(c):
            for d in range(rows.shape[1]):
                out[i, d, s] = rows[r, d]
            r += 1
    return out


@pytest.mark.parametrize("ft", ["f32", "f16", "bf16", "e4m3", "e5m2"])
def test_unpack_regions_is_the_plain_loop(ft):
    S, D = 9, 4
    counts = [9, 1, 4, 9, 5, 1]                                 # 1 and S among them
    rng = np.random.default_rng(1)
    vals = rng.uniform(-3, 3, (sum(counts), D)).astype(np.float32)
    vals[0, 0], vals[3, 1] = -0.0, 0.0                          # zeros of either sign are values like any other
    rows = np.empty(vals.shape, feat16.dtype_of(ft))
    feat16.store(rows, vals, ft)
    dense = feat16.unpack_regions(rows, counts, S)
    assert dense.dtype == rows.dtype and dense.shape == (len(counts), D, S)
    assert dense.tobytes() == plain_loop(rows, counts, S).tobytes()
    for i, c in enumerate(counts):
        assert not dense[i, :, c:].view(np.uint8).any()         # all bits zero behind the count: +0 in every type
    assert dense[0, 0, 0].tobytes() == rows[0, 0].tobytes() and any(rows[0, 0].tobytes())   # -0 keeps its sign


@pytest.mark.parametrize("bad", [[0, 3], [3, 10], [-1, 3], [], [[2, 2]], [1.5, 2.0]])
def test_unpack_regions_rejects_bad_counts(bad):
    n = int(np.sum(np.clip(np.asarray(bad, np.float64), 0, None)))
    with pytest.raises(ValueError):
        feat16.unpack_regions(np.zeros((max(n, 1), 4), np.float32), bad, 9)


def test_unpack_regions_rejects_rows_that_do_not_match():
    with pytest.raises(ValueError):
        feat16.unpack_regions(np.zeros((6, 4), np.float32), [3, 4], 9)
    with pytest.raises(ValueError):
        feat16.unpack_regions(np.zeros(28, np.float32), [3, 4], 9)


# ---------------------------------------------------------------- loader
N, T, D, W, H, NIMG, B = 24, 5, 4, 3, 3, 6, 8
S = W * H
IMG = [1, 2, 1, 3, 2, 1, 4, 3,   5, 5, 6, 5, 1, 6, 2, 1,   3, 3, 3, 3, 3, 3, 3, 3]
BOXES_PER_IMAGE = [9, 1, 4, 7, 9, 2]                            # 1 and S among them
HALF = (1, 4)                                                   # images stored as HalfTensor files


@pytest.fixture()
def data(tmp_path):
    """The same boxes twice, with t7's own writer: region files [n, D] and dense files [D, W, H] padded with zeros."""
    rng = np.random.default_rng(3)
    names = [f"val2014/COCO_val2014_{i:012d}.jpg" for i in range(NIMG)]
    rdir, ddir = tmp_path / "regions", tmp_path / "dense"
    rdir.mkdir()
    ddir.mkdir()
    for k, (name, n) in enumerate(zip(names, BOXES_PER_IMAGE)):
        boxes = rng.standard_normal((n, D)).astype(np.float32)
        if k in HALF:
            boxes = boxes.astype(np.float16)
        dense = np.zeros((D, S), boxes.dtype)
        dense[:, :n] = boxes.T
        t7.save(rdir / loader.feature_name(name), boxes)
        t7.save(ddir / loader.feature_name(name), dense.reshape(D, W, H))
    lens = rng.integers(1, T + 1, N)
    q = np.zeros((N, T), np.int32)
    for i, l in enumerate(lens):
        q[i, :l] = rng.integers(2, 9, l)
    ans = rng.integers(1, 11, N)

    def make(feat_type="f32", prefetch=False):
        qs = loader.QuestionSet(question=q, lengths_q=lens, img_list=np.array(IMG), question_id=np.arange(N),
                                answers=ans)
        return loader.DataClass(qs, names, B, "train", prefetch=prefetch, feat_type=feat_type)
    return make, str(rdir), str(ddir)


def test_load_regions_reads_2d_tensors(data, tmp_path):
    make, rdir, ddir = data
    p = os.path.join(rdir, "COCO_val2014_000000000001.t7")
    assert t7.load_regions(p, D).dtype == np.float32 and t7.load_regions(p, D).shape == (1, D)
    assert t7.load_regions(p, D, keep_half=True).dtype == np.float16          # a HalfTensor file
    with pytest.raises(t7.T7Error):
        t7.load_regions(p, D + 4)
    with pytest.raises(t7.T7Error):
        t7.load_regions(os.path.join(ddir, "COCO_val2014_000000000001.t7"), D)   # a 3-D map is not region rows


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("unique", [False, True])
@pytest.mark.parametrize("ft", ["f32", "f16", "bf16", "e4m3"])
def test_packed_batches_unpack_to_the_dense_ones(data, ft, unique, prefetch):
    make, rdir, ddir = data
    dense, packed = make(ft), make(ft, prefetch=prefetch)
    for k in range(4):                                          # the fourth is the first of the next epoch
        want = dense.next_batch_feat(ddir, D, W, H, unique=unique)
        got = packed.next_batch_feat(rdir, D, W, H, unique=unique, packed=True)
        assert len(got) == len(want) + 1
        rows, counts = got[:2]
        img = IMG[(k % 3) * B:(k % 3 + 1) * B]
        per = list(dict.fromkeys(img)) if unique else img
        assert counts.dtype == np.int32 and counts.tolist() == [BOXES_PER_IMAGE[i - 1] for i in per]
        assert rows.dtype == feat16.dtype_of(ft) and rows.shape == (int(counts.sum()), D)
        assert feat16.unpack_regions(rows, counts, S).tobytes() == want[0].tobytes()
        for u, v in zip(got[2:], want[1:]):
            np.testing.assert_array_equal(u, v)


def test_each_region_file_is_read_once_and_nothing_is_padded(data, monkeypatch):
    make, rdir, _ = data
    seen = []
    real = t7.load_regions
    monkeypatch.setattr(t7, "load_regions", lambda p, *a, **k: (seen.append(str(p)), real(p, *a, **k))[1])
    rows, counts = make().next_batch_feat(rdir, D, W, H, unique=True, packed=True)[:2]
    assert len(seen) == 4 and len(set(seen)) == 4
    assert rows.shape[0] == 9 + 1 + 4 + 7 < 4 * S
    with pytest.raises(ValueError):
        make().next_batch_feat(rdir, D, 2, 2, packed=True)      # a file with more boxes than S


def test_prefetch_into_a_staging_buffer_packs_at_its_start(data):
    make, rdir, ddir = data
    d = make(prefetch=True)
    stage, other = np.full((B, D, S), 7.0, np.float32), np.zeros((B, D, S), np.float32)
    dests = [stage, other]
    d._next_dest = lambda: dests.pop(0)
    d.next_batch_feat(rdir, D, W, H, packed=True)               # starts the worker for batch 1
    rows, counts = d.next_batch_feat(rdir, D, W, H, packed=True)[:2]
    assert np.shares_memory(rows, stage) and rows.ctypes.data == stage.ctypes.data
    ref = make()
    ref.next_batch_feat(ddir, D, W, H)
    assert feat16.unpack_regions(rows, counts, S).tobytes() == ref.next_batch_feat(ddir, D, W, H)[0].tobytes()
    assert (stage.reshape(-1)[rows.size:] == 7.0).all()         # nothing beyond the rows is touched


class _FakeRau:
    """The calls SlotFeeder, fill_bank and feed make, on ordinary memory."""

    def __init__(self, bank_type="f32"):
        self.stage = [{"feats": np.zeros((B, D, S), np.float32), "tokens": np.zeros((T, B), np.int32),
                       "lens": np.zeros(B, np.int32), "labels": np.zeros(B, np.int32)} for _ in range(2)]
        self.uploads, self.current, self.bank, self.bank_type, self.fed = [], None, {}, bank_type, None

    def batch_slot(self, slot, feat_type="f32"):
        return self.stage[slot]

    def set_batch_async(self, slot, has_labels=True, image_of=None, packed_counts=None, **kw):
        assert "n_images" not in kw and "feats" not in kw
        s = self.stage[slot]
        n = int(packed_counts.sum())
        self.uploads.append((slot, s["feats"].reshape(-1)[:n * D].reshape(n, D).copy(), packed_counts.copy(),
                             None if image_of is None else image_of.copy(), s["tokens"].copy()))

    def set_regions(self, *a, **k):
        raise AssertionError("a packed batch brings its own counts")

    def use_batch(self, slot):
        self.current = slot

    def bank_info(self):
        return {"capacity": NIMG, "feat_type": self.bank_type, "rows_filled": len(self.bank)}

    def bank_put_packed(self, first, rows, counts, feat_type=None):
        maps = feat16.unpack_regions(rows, counts, S)
        for i in range(len(counts)):
            self.bank[first + i] = maps[i]

    def set_batch_packed(self, rows, counts, x, x_len, labels=None, feat_type=None, image_of=None):
        self.fed = (rows, counts, x, x_len, labels, feat_type, image_of)


@pytest.mark.parametrize("share", [False, True])
def test_slot_feeder_assembles_the_rows_in_the_staging(data, share):
    make, rdir, ddir = data
    rau = _FakeRau()
    qs_regions = make()
    qs_regions.qs.img_regions = np.array(BOXES_PER_IMAGE, np.int32)   # must not be sent a second time
    feeder = loader.SlotFeeder(rau, qs_regions, rdir, D, W, H, share_images=share, packed=True)
    feeder.next()
    feeder.next()
    ref = make()
    assert [u[0] for u in rau.uploads] == [0, 1, 0] and rau.current == 0
    for slot, rows, counts, image_of, tokens in rau.uploads:
        f, x = ref.next_batch_feat(ddir, D, W, H)[:2]
        maps = feat16.unpack_regions(rows, counts, S)
        assert (image_of is not None) == share
        np.testing.assert_array_equal((maps[image_of] if share else maps).reshape(f.shape), f)
        np.testing.assert_array_equal(tokens, x)


def test_fill_bank_packed_fills_the_bank_and_the_image_counts(data):
    make, rdir, ddir = data
    rau, d = _FakeRau(), make()
    regions = d.fill_bank(rau, rdir, D, W, H, chunk=4, packed=True)
    assert regions.tolist() == BOXES_PER_IMAGE and d.qs.img_regions is regions
    files, _ = d.bank_rows(rdir)
    ref = make()
    for r, p in enumerate(files):
        want = t7.load_feature(os.path.join(ddir, os.path.basename(p)), D, W, H)
        np.testing.assert_array_equal(rau.bank[r], want)
    rows, image_of = d.next_batch_rows(rdir)[:2]
    assert d.last_regions.tolist() == [BOXES_PER_IMAGE[i - 1] for i in IMG[:B]]   # per sample, for set_regions


def test_feed_accepts_a_packed_batch(data):
    make, rdir, _ = data
    rau = _FakeRau()
    batch = make().next_batch_feat(rdir, D, W, H, unique=True, packed=True)
    qids = loader.feed(rau, batch)
    np.testing.assert_array_equal(qids, batch[5])
    assert rau.fed[0] is batch[0] and rau.fed[1] is batch[1] and rau.fed[6] is batch[6] and rau.fed[4] is batch[4]
    loader.feed(rau, make("bf16").next_batch_feat(rdir, D, W, H, packed=True), feat_type="bf16")
    assert rau.fed[5] == "bf16" and rau.fed[6] is None and rau.fed[0].dtype == np.uint16


# ---------------------------------------------------------------- the GPU tests' shapes against the tile constants
def tile_constants():
    text = open(os.path.join(ROOT, "rau_vqa_amd", "csrc", "packed.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (kPack\w+) = (\d+);", text)}


def test_the_gpu_shapes_straddle_every_edge_of_the_unpack_tile():
    from tests.test_gpu_packed import KERNEL_CASES, SHAPES
    k = tile_constants()
    TD, TS, QUAD = k["kPackTileD"], k["kPackTileS"], 4
    assert (TD, TS, k["kPackPitch"]) == (64, 64, 18)            # the table below is written for these
    assert TS % QUAD == 0 and TD % QUAD == 0
    cases = {name: (dims["D"], dims["S"], counts) for name, (dims, counts) in SHAPES.items()}
    assert {n for n, _ in KERNEL_CASES} == set(cases)           # every shape of the table runs
    for D_, S_, counts in cases.values():
        assert all(1 <= c <= S_ for c in counts) and len(counts) >= 2 and D_ % 4 == 0

    def some(pred):
        return any(pred(D_, S_, c) for D_, S_, counts in cases.values() for c in counts)
    # positions: a count below, at, just above and far above the tile edge, where a second tile exists
    assert some(lambda D_, S_, c: S_ > TS and c < TS)
    assert some(lambda D_, S_, c: S_ > TS and c == TS)
    assert some(lambda D_, S_, c: S_ > TS and c > TS and c % QUAD)
    assert some(lambda D_, S_, c: S_ > TS and c == S_)
    assert some(lambda D_, S_, c: S_ <= TS and c == S_)
    # quads: counts that end inside one and on one; 1; the last full quad in front of a pad quad; S inside the pad quad
    assert some(lambda D_, S_, c: c % QUAD == 0 and c < S_) and some(lambda D_, S_, c: c % QUAD in (1, 2, 3) and c < S_)
    assert some(lambda D_, S_, c: c == 1)
    assert some(lambda D_, S_, c: S_ % QUAD and c == S_) and some(lambda D_, S_, c: S_ % QUAD and c == S_ // QUAD * QUAD)
    assert some(lambda D_, S_, c: S_ == QUAD)
    # channels: one partial tile, one and two full tiles plus a partial one, many full tiles
    widths = {D_ for D_, _, _ in cases.values()}
    assert any(D_ < TD for D_ in widths) and TD + 4 in widths and 2 * TD + 4 in widths
    assert any(D_ % TD == 0 and D_ >= 4 * TD for D_ in widths)
    # all five element types at the shape with two position tiles; the 4- and 1-byte movers elsewhere
    assert {ft for n, ft in KERNEL_CASES if n == "boxes"} == {"f32", "f16", "bf16", "e4m3", "e5m2"}
    for n in cases:
        assert {"f32", "e4m3"} <= {ft for m, ft in KERNEL_CASES if m == n}, n
