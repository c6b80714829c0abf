"""The feature bank on the host side: the loader names every distinct image of a split by a bank row,
fills a bank reading each file once, and hands out batches of rows that stand for exactly the maps
next_batch_feat would have read; librau.so exports the bank entry points."""
import ctypes as C

import numpy as np
import pytest

from rau_vqa_amd import feat16, loader, t7

N, T, D, W, H, NIMG, B = 24, 5, 4, 2, 2, 6, 8
# image of every question: repeats inside a batch, NOT adjacent, and a batch (the third) of one image only
IMG = [1, 2, 1, 3, 2, 1, 4, 3,   5, 5, 6, 5, 1, 6, 2, 1,   3, 3, 3, 3, 3, 3, 3, 3]
BANK_SYMBOLS = ("rau_bank_create", "rau_bank_destroy", "rau_bank_info", "rau_bank_put", "rau_bank_get",
                "rau_set_batch_bank", "rau_set_batch_async_bank")


@pytest.fixture()
def data(tmp_path):
    rng = np.random.default_rng(3)
    names = [f"val2014/COCO_val2014_{i:012d}.jpg" for i in range(NIMG)]
    fdir = tmp_path / "feat"
    fdir.mkdir()
    for k, name in enumerate(names):
        a = rng.standard_normal((D, W, H)).astype(np.float32)
        # images 2 and 5 are stored as HalfTensor files: they go into an fp16 bank as they are
        t7.save(fdir / loader.feature_name(name), a.astype(np.float16) if k in (1, 4) else a)
    lens = rng.integers(1, T + 1, N)
    q = np.zeros((N, T), np.int32)
    for i, l in enumerate(lens):
        q[i, :l] = rng.integers(2, 9, l)
    ans = rng.integers(1, 11, N)

    def make(feat_type="f32"):
        qs = loader.QuestionSet(question=q, lengths_q=lens, img_list=np.array(IMG), question_id=np.arange(N),
                                answers=ans)
        return loader.DataClass(qs, names, B, "train", feat_type=feat_type)
    return make, str(fdir)


class _FakeRau:
    """A bank in ordinary memory with rau_bank_put's conversion rules (f32 into a 16-bit bank is narrowed
    as feat16.store does), and the slot calls SlotFeeder makes."""

    def __init__(self, feat_type="f32", capacity=NIMG):
        self.ft = feat_type
        self.bank = np.zeros((capacity, D, W * H), feat16.dtype_of(feat_type))
        self.written = np.zeros(capacity, bool)
        self.puts = []
        self.stage = [{"feats": np.full((B, D, W * H), 7.0, np.float32), "tokens": np.zeros((T, B), np.int32),
                       "lens": np.zeros(B, np.int32), "labels": np.zeros(B, np.int32)} for _ in range(2)]
        self.uploads, self.current = [], None

    def bank_info(self):
        return {"capacity": len(self.bank), "feat_type": self.ft, "rows_filled": int(self.written.sum())}

    def bank_put(self, first, feats, feat_type=None):
        feats = np.asarray(feats)
        src = feat16.infer(feats, feat_type)
        assert src == self.ft or src == "f32", (src, self.ft)
        n = feats.shape[0]
        feat16.store(self.bank[first:first + n], feats.reshape(n, D, W * H))
        self.written[first:first + n] = True
        self.puts.append((first, n, src))

    def batch_slot(self, slot, feat_type="f32"):
        return self.stage[slot]

    def set_batch_async(self, slot, has_labels=True, bank_rows=None, image_of=None, **kw):
        assert not kw, kw                                         # no feats, no feat_type, no n_images
        s = self.stage[slot]
        self.uploads.append((slot, bank_rows.copy(), image_of.copy(), s["tokens"].copy(), s["lens"].copy(),
                             s["labels"].copy()))

    def use_batch(self, slot):
        self.current = slot


def test_library_exports_the_bank_entry_points():
    from rau_vqa_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in BANK_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib._SIGS, name


def test_bank_rows_is_deterministic_and_covers_each_file_once(data):
    make, fdir = data
    d = make()
    files, row_of = d.bank_rows(fdir)
    assert len(files) == NIMG == len(set(files)) and sorted(row_of.values()) == list(range(NIMG))
    assert [row_of[f] for f in files] == list(range(NIMG))
    # order: first question of each image in the DATA SET, whatever the batch order is
    assert [int(f[-6:-3]) for f in files] == [i - 1 for i in dict.fromkeys(IMG)]
    shuffled = make()
    shuffled.set_batch_order_option(1)
    shuffled.reorder()
    assert shuffled.bank_rows(fdir) == (files, row_of)
    assert d.bank_rows([fdir]) == (files, row_of)             # a path or a list of paths


@pytest.mark.parametrize("ft", ["f32", "f16", "bf16"])
def test_fill_bank_reads_each_file_once(data, monkeypatch, ft):
    make, fdir = data
    seen = []
    real = t7.load_feature
    monkeypatch.setattr(t7, "load_feature", lambda p, *a, **k: (seen.append(str(p)), real(p, *a, **k))[1])
    d, rau = make(ft), _FakeRau(ft)
    assert d.fill_bank(rau, fdir, D, W, H, chunk=4) == NIMG
    assert seen == d.bank_rows(fdir)[0]                        # each distinct file once, in row order
    assert rau.written.all() and [p[:2] for p in rau.puts] == [(0, 4), (4, 2)]
    # f32 files go up as f32 (narrowed by the bank); a chunk of HalfTensor files only would go up as f16
    assert all(p[2] == "f32" for p in rau.puts)
    with pytest.raises(ValueError):
        d.fill_bank(_FakeRau(ft, capacity=NIMG - 1), fdir, D, W, H)


def test_half_files_go_into_an_fp16_bank_as_they_are(data):
    make, fdir = data
    d, rau = make("f16"), _FakeRau("f16")
    d.fill_bank(rau, fdir, D, W, H, chunk=1)
    assert [p[2] for p in rau.puts] == ["f32", "f16", "f32", "f32", "f16", "f32"]
    f32 = _FakeRau("f32")
    make().fill_bank(f32, fdir, D, W, H, chunk=1)              # an f32 bank takes every file widened
    assert all(p[2] == "f32" for p in f32.puts)


@pytest.mark.parametrize("ft", ["f32", "f16", "bf16"])
def test_bank_batches_are_next_batch_feat_bit_for_bit(data, monkeypatch, ft):
    make, fdir = data
    ref, d, rau = make(ft), make(ft), _FakeRau(ft)
    d.fill_bank(rau, fdir, D, W, H)
    seen = []
    real = t7.load_feature
    batches = [ref.next_batch_feat(fdir, D, W, H, unique=True) for _ in range(4)]   # 3 batches + the epoch wrap
    plain = make(ft)
    plains = [plain.next_batch_feat(fdir, D, W, H) for _ in range(4)]
    monkeypatch.setattr(t7, "load_feature", lambda p, *a, **k: (seen.append(str(p)), real(p, *a, **k))[1])
    for k in range(4):
        out = d.next_batch_rows(fdir)
        assert len(out) == 6
        rows, image_of, x, xl, a, qid = out
        tf, tx, txl, ta, tqid, timage_of = batches[k]
        assert rows.dtype == np.int32 and image_of.dtype == np.int32 and image_of.shape == (B,)
        np.testing.assert_array_equal(image_of, timage_of)
        assert rau.bank[rows].tobytes() == tf.reshape(len(rows), D, W * H).tobytes()       # the table
        assert rau.bank[rows][image_of].tobytes() == plains[k][0].tobytes()                 # the plain batch
        for u, v in ((x, tx), (xl, txl), (a, ta), (qid, tqid)):
            assert u.dtype == v.dtype
            np.testing.assert_array_equal(u, v)
    assert len(batches[2][0]) == 1 and len(d.next_batch_rows(fdir)[0]) == 4   # N = 1; batch 1 of the second epoch
    assert not seen                                            # no file is opened


def test_feed_hands_a_rows_tuple_to_set_batch(data):
    make, fdir = data
    d = make()
    calls = []

    class R:
        def set_batch(self, feats, tokens, lens, labels=None, **kw):
            calls.append((feats, tokens, lens, labels, kw))
    batch = d.next_batch_rows(fdir)
    qids = loader.feed(R(), batch)
    np.testing.assert_array_equal(qids, batch[5])
    feats, tokens, lens, labels, kw = calls[0]
    assert feats is None and sorted(kw) == ["bank_rows", "image_of"]
    np.testing.assert_array_equal(kw["bank_rows"], batch[0])
    np.testing.assert_array_equal(kw["image_of"], batch[1])
    np.testing.assert_array_equal(labels, batch[4])


def test_slot_feeder_drives_the_slots_with_rows(data, monkeypatch):
    make, fdir = data
    rau = _FakeRau()
    d = make()
    d.fill_bank(rau, fdir, D, W, H)
    with monkeypatch.context() as mp:
        mp.setattr(t7, "load_feature", lambda *a, **k: pytest.fail("a bank feeder opens no feature file"))
        feeder = loader.SlotFeeder(rau, d, fdir, D, W, H, bank=True)
        feeder.next()
        qids = feeder.next()
    assert d._job is None                                     # no prefetch worker
    assert [u[0] for u in rau.uploads] == [0, 1, 0] and rau.current == 0
    ref = make()
    for slot, rows, image_of, tokens, lens, labels in rau.uploads:
        f, x, xl, a, q = ref.next_batch_feat(fdir, D, W, H)
        np.testing.assert_array_equal(rau.bank[rows][image_of], f.reshape(B, D, W * H))
        np.testing.assert_array_equal(tokens, x)
        np.testing.assert_array_equal(lens, xl)
        np.testing.assert_array_equal(labels, a)
    np.testing.assert_array_equal(qids, q)
    for s in rau.stage:
        assert (s["feats"] == 7.0).all()                      # the feature staging is never written
