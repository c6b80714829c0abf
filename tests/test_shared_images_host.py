"""Image tables on the host side: next_batch_feat(unique=True) reads every distinct feature file of a
batch once and returns the table + the 0-based index, such that feats[image_of] is the plain batch
bit for bit; librau.so exports the three table entry points."""
import ctypes as C

import numpy as np
import pytest

from rau_vqa_amd import feat16, loader, t7

N, T, D, W, H, NIMG, B = 24, 5, 4, 2, 2, 6, 8
# image of every question: repeats inside a batch, NOT adjacent, and a batch (the third) of one image only
IMG = [1, 2, 1, 3, 2, 1, 4, 3,   5, 5, 6, 5, 1, 6, 2, 1,   3, 3, 3, 3, 3, 3, 3, 3]


@pytest.fixture()
def data(tmp_path):
    rng = np.random.default_rng(3)
    names = [f"val2014/COCO_val2014_{i:012d}.jpg" for i in range(NIMG)]
    fdir = tmp_path / "feat"
    fdir.mkdir()
    for name in names:
        t7.save(fdir / loader.feature_name(name), rng.standard_normal((D, W, H)).astype(np.float32))
    lens = rng.integers(1, T + 1, N)
    q = np.zeros((N, T), np.int32)
    for i, l in enumerate(lens):
        q[i, :l] = rng.integers(2, 9, l)
    ans = rng.integers(1, 11, N)

    def make(feat_type="f32", prefetch=False):
        qs = loader.QuestionSet(question=q, lengths_q=lens, img_list=np.array(IMG), question_id=np.arange(N),
                                answers=ans)
        return loader.DataClass(qs, names, B, "train", prefetch=prefetch, feat_type=feat_type)
    return make, str(fdir)


@pytest.mark.parametrize("ft", ["f32", "f16", "bf16"])
def test_table_expands_to_the_plain_batch(data, ft):
    make, fdir = data
    plain, uniq = make(ft), make(ft)
    for k in range(3):
        f, x, xl, a, qid = plain.next_batch_feat(fdir, D, W, H)
        out = uniq.next_batch_feat(fdir, D, W, H, unique=True)
        assert len(out) == 6
        tf, tx, txl, ta, tqid, image_of = out
        img = IMG[k * B:(k + 1) * B]
        first = list(dict.fromkeys(img))                      # distinct images in order of first appearance
        assert tf.shape == (len(first), D, W, H) and tf.dtype == feat16.dtype_of(ft)
        assert image_of.dtype == np.int32 and image_of.shape == (B,)
        np.testing.assert_array_equal(image_of, [first.index(i) for i in img])
        assert tf[image_of].tobytes() == f.tobytes()          # bit for bit, in the batch's element type
        for u, v in ((x, tx), (xl, txl), (a, ta), (qid, tqid)):
            np.testing.assert_array_equal(u, v)
    assert len(first) == 1                                    # the last batch: N = 1


def test_each_distinct_file_is_read_once(data, monkeypatch):
    make, fdir = data
    seen = []
    real = t7.load_feature
    monkeypatch.setattr(t7, "load_feature", lambda p, *a, **k: (seen.append(str(p)), real(p, *a, **k))[1])
    d = make()
    d.next_batch_feat(fdir, D, W, H, unique=True)
    assert len(seen) == 4 and len(set(seen)) == 4             # images 1, 2, 3, 4
    assert [int(s[-6:-3]) for s in seen] == [0, 1, 2, 3]      # order of first appearance
    seen.clear()
    d.next_batch_feat(fdir, D, W, H)                          # the plain call reads one file per question
    assert len(seen) == B


def test_unique_false_is_the_old_tuple(data):
    make, fdir = data
    out = make().next_batch_feat(fdir, D, W, H, unique=False)
    assert len(out) == 5 and out[0].shape == (B, D, W, H)
    assert len(make().next_batch_feat(fdir, D, W, H)) == 5


def test_prefetched_table_equals_the_synchronous_one(data, monkeypatch):
    make, fdir = data
    sync, pre = make(), make(prefetch=True)
    seen = []
    real = t7.load_feature
    monkeypatch.setattr(t7, "load_feature", lambda p, *a, **k: (seen.append(str(p)), real(p, *a, **k))[1])
    for k in range(3):
        a = sync.next_batch_feat(fdir, D, W, H, unique=True)
        seen.clear()
        b = pre.next_batch_feat(fdir, D, W, H, unique=True)
        if k:                                                 # batches 1.. came from the worker: no file read here
            pre._job[1].join()
            assert len(seen) == len(set(seen))                # and the worker reads each file of the NEXT batch once
        assert len(b) == 6
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


def test_prefetch_into_a_staging_buffer_fills_its_first_maps(data):
    """SlotFeeder's arrangement: the worker assembles the table at the start of a [B,D,S] destination."""
    make, fdir = data
    d = make(prefetch=True)
    stage, other = np.full((B, D, W * H), 7.0, np.float32), np.zeros((B, D, W * H), np.float32)
    dests = [stage, other]                                    # as the feeder does: the worker alternates slots
    d._next_dest = lambda: dests.pop(0)
    d.next_batch_feat(fdir, D, W, H, unique=True)             # starts the worker for batch 1 (images 5, 6, 1, 2)
    tf, _, _, _, _, image_of = d.next_batch_feat(fdir, D, W, H, unique=True)
    assert np.shares_memory(tf, stage) and tf.shape == (4, D, W, H)
    ref = make()
    ref.next_batch_feat(fdir, D, W, H)
    np.testing.assert_array_equal(tf[image_of], ref.next_batch_feat(fdir, D, W, H)[0])
    assert (stage[4:] == 7.0).all()                           # nothing beyond the N maps is touched


def test_library_exports_the_table_entry_points():
    from rau_vqa_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("rau_set_batch_images", "rau_set_batch_async_images", "rau_batch_images"):
        assert hasattr(lib, name), name
        assert name in _lib._SIGS


class _FakeRau:
    """The three slot calls SlotFeeder makes, on ordinary memory."""

    def __init__(self):
        self.stage = [{"feats": np.zeros((B, D, W * H), np.float32), "tokens": np.zeros((T, B), np.int32),
                       "lens": np.zeros(B, np.int32), "labels": np.zeros(B, np.int32)} for _ in range(2)]
        self.uploads, self.current = [], None

    def batch_slot(self, slot, feat_type="f32"):
        return self.stage[slot]

    def set_batch_async(self, slot, has_labels=True, image_of=None, n_images=None, **kw):
        s = self.stage[slot]
        self.uploads.append((slot, s["feats"].reshape(-1)[:n_images * D * W * H].reshape(n_images, D, W, H).copy(),
                             image_of.copy(), s["tokens"].copy()))

    def use_batch(self, slot):
        self.current = slot


def test_slot_feeder_shares_images(data):
    make, fdir = data
    rau = _FakeRau()
    feeder = loader.SlotFeeder(rau, make(), fdir, D, W, H, share_images=True)
    feeder.next()
    feeder.next()
    ref = make()
    assert [u[0] for u in rau.uploads] == [0, 1, 0] and rau.current == 0
    for slot, table, image_of, tokens in rau.uploads:
        f, x, _, _, _ = ref.next_batch_feat(fdir, D, W, H)
        assert table.shape[0] == len(set(image_of.tolist())) and image_of.dtype == np.int32
        np.testing.assert_array_equal(table[image_of], f)      # the first N maps of the staging are the table
        np.testing.assert_array_equal(tokens, x)
