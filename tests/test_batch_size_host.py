"""rau_set_batch_size on the host side: header, Lua cdef and ctypes table declare the two entry points alike;
the Python driver checks sizes and row counts before anything reaches the library and follows the current
size in every shape; loader.feed and SlotFeeder run a test split whose batch size is below the capacity."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rau_vqa_amd import _lib, loader, t7
from rau_vqa_amd.model import RAU, Config
from tests.test_abi import ROOT, _normalise

SYMBOLS = ("rau_set_batch_size", "rau_batch_size")
DIMS = dict(B=8, T=5, V=30, E=8, Rq=4, D=4, S=4, M=8, A=4, R=4, K=10, H=2)


def _proto(text, name):
    m = re.search(r"\bint\s+" + name + r"\s*\([^;]*\)\s*;", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    assert m, name
    return _normalise(m.group(0))


def test_header_lua_and_ctypes_declare_the_same_signatures():
    header = open(os.path.join(ROOT, "include", "rau.h")).read()
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    want = {"rau_set_batch_size": "int rau_set_batch_size(rau_ctx* ctx, int32_t n);",
            "rau_batch_size": "int rau_batch_size(rau_ctx* ctx, int32_t* n, int32_t* capacity);"}
    for name in SYMBOLS:
        assert _proto(header, name) == _proto(lua, name) == want[name]
    assert _lib._SIGS["rau_set_batch_size"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert _lib._SIGS["rau_batch_size"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)])
    assert "function RAU:setBatchSize(n)" in lua and "function RAU:batchSize()" in lua
    assert "#define RAU_ABI_VERSION 5" in header            # additive, like the bank and image-table calls


def test_library_exports_the_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    # both reject a null context before they look at anything else (no device needed)
    l = _lib.lib()
    assert l.rau_set_batch_size(None, 4) == -1
    assert l.rau_batch_size(None, None, None) == -1


class _RecLib:
    """Stands in for librau.so: records every call, succeeds, writes nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name,) + args[1:])
            return 0
        return fn


def _rau(**over):
    m = RAU.__new__(RAU)
    m.cfg = Config(**dict(DIMS, **over))
    m._lib, m._h, m._n = _RecLib(), None, m.cfg.B
    return m


def _batch(n, d=DIMS):
    rng = np.random.default_rng(n)
    return dict(feats=rng.standard_normal((n, d["D"], d["S"])).astype(np.float32),
                tokens=rng.integers(1, d["V"], (d["T"], n)).astype(np.int32),
                lens=rng.integers(0, d["T"] + 1, n).astype(np.int32),
                labels=rng.integers(1, d["K"] + 1, n).astype(np.int32))


def test_set_batch_size_validates_before_the_library_is_called():
    m = _rau()
    assert (m.batch_size, m.capacity) == (8, 8)
    for bad in (0, -1, 9):
        with pytest.raises(ValueError):
            m.set_batch_size(bad)
    assert m._lib.calls == [] and m.batch_size == 8
    m.set_batch_size(5)
    assert m._lib.calls == [("rau_set_batch_size", 5)] and (m.batch_size, m.capacity, m.cfg.B) == (5, 8, 8)


def test_set_batch_infers_the_size_and_rejects_mismatched_rows():
    m = _rau()
    b5, b8, b9 = _batch(5), _batch(8), _batch(9)
    with pytest.raises(ValueError):                           # above the capacity
        m.set_batch(**b9)
    for k in ("feats", "tokens", "labels"):                   # one array of another row count
        with pytest.raises(ValueError):
            m.set_batch(**dict(b5, **{k: b8[k]}))
    with pytest.raises(ValueError):
        m.set_batch(b5["feats"][:2], b5["tokens"], b5["lens"], b5["labels"], image_of=np.zeros(8, np.int32))
    with pytest.raises(ValueError):
        m.set_batch(None, b5["tokens"], b5["lens"], b5["labels"], bank_rows=np.arange(8))
    with pytest.raises(ValueError):
        m.set_batch_async(0, b5["feats"], b8["tokens"], b5["lens"], b5["labels"])
    with pytest.raises(ValueError):
        m.set_batch_async(0, lens=b9["lens"])
    assert m._lib.calls == [] and m.batch_size == 8           # nothing reached the library
    m.set_batch(**b5)                                         # switches, then hands the batch over
    assert [c[0] for c in m._lib.calls] == ["rau_set_batch_size", "rau_set_batch_typed"]
    assert m._lib.calls[0] == ("rau_set_batch_size", 5) and m.batch_size == 5
    m.set_batch(**b5)                                         # same size: no second switch
    assert [c[0] for c in m._lib.calls].count("rau_set_batch_size") == 1
    m.set_batch(None, b8["tokens"], b8["lens"], b8["labels"], bank_rows=np.arange(8))     # back, as a bank batch
    assert [c[0] for c in m._lib.calls][-2:] == ["rau_set_batch_size", "rau_set_batch_bank"] and m.batch_size == 8
    m.set_batch_async(1, b5["feats"], b5["tokens"], b5["lens"], b5["labels"])
    assert [c[0] for c in m._lib.calls][-2:] == ["rau_set_batch_size", "rau_set_batch_async_typed"]
    m.set_batch_async(0, has_labels=False)                    # staging filled in place: the current size
    assert m.batch_size == 5 and m._lib.calls[-1][0] == "rau_set_batch_async_typed"


def test_result_shapes_follow_the_current_size():
    m = _rau()
    m.set_batch_size(3)
    c = m.cfg
    assert m.argmax().shape == (c.H, 3) and m.logits().shape == (c.H, 3, c.K)
    assert m.dopred().shape == (c.H, 3) and m.attention().shape == (c.H, 3, c.S)
    assert m.question_state().shape == (3, c.Q) and m.att_state()[0].shape == (c.H, 3, c.R)
    assert m.losses().shape == (c.H,)
    oe, mc = m.predict(np.zeros((3, 4), np.int32))
    assert oe.shape == mc.shape == (c.H + 2, 3)
    with pytest.raises(ValueError):
        m.predict(np.zeros((8, 4), np.int32))                 # an MC list of the capacity's rows
    pred, att = m.merged()
    assert pred.shape == (2, 3, c.K) and att.shape == (2, 3, c.S)
    assert m.cfg.mask_shapes(3)["x"] == (c.H, 3, c.D, c.S) and m.cfg.mask_shapes()["x"] == (c.H, 8, c.D, c.S)


# ---- loader: a test split at test_batch_size < capacity
N, T, D, W, H, NIMG, CAP, TB = 12, 5, 4, 2, 2, 4, 8, 3


@pytest.fixture()
def split(tmp_path):
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
    qs = loader.QuestionSet(question=q, lengths_q=lens, img_list=rng.integers(1, NIMG + 1, N),
                            question_id=np.arange(N), mc_ans=rng.integers(0, 11, (N, 4)))
    return (lambda: loader.DataClass(qs, names, TB, "test")), str(fdir)


class _SizedRau:
    """The calls feed and SlotFeeder make, with the driver's size rules: capacity CAP, current size n."""

    def __init__(self):
        self.capacity, self.batch_size, self.resizes = CAP, CAP, []
        self.batches, self.uploads, self.current = [], [], None
        self._stage()

    def _stage(self):
        n = self.batch_size
        self.stage = [{"feats": np.zeros((n, D, W * H), np.float32), "tokens": np.zeros((T, n), np.int32),
                       "lens": np.zeros(n, np.int32), "labels": np.zeros(n, np.int32)} for _ in range(2)]

    def set_batch_size(self, n):
        if not 1 <= n <= self.capacity:
            raise ValueError(n)
        self.resizes.append(n)
        self.batch_size = n
        self._stage()

    def set_batch(self, feats, tokens, lens, labels=None, **kw):
        if lens.shape[0] != self.batch_size:
            self.set_batch_size(lens.shape[0])
        self.batches.append((feats, tokens, lens, labels))

    def batch_slot(self, slot, feat_type="f32"):
        return self.stage[slot]

    def set_batch_async(self, slot, has_labels=True, **kw):
        s = self.stage[slot]
        self.uploads.append((slot, has_labels, s["feats"].copy(), s["tokens"].copy(), s["lens"].copy()))

    def use_batch(self, slot):
        self.current = slot


def test_feed_takes_a_test_batch_below_the_capacity(split):
    make, fdir = split
    d, rau = make(), _SizedRau()
    batch = d.next_batch_feat(fdir, D, W, H)
    qids = loader.feed(rau, batch)
    feats, tokens, lens, labels = rau.batches[0]
    assert rau.resizes == [TB] and feats.shape == (TB, D, W * H) and tokens.shape == (T, TB)
    assert lens.shape == (TB,) and labels is None and len(qids) == TB


def test_slot_feeder_is_bound_to_its_batch_size(split):
    make, fdir = split
    d, rau = make(), _SizedRau()
    feeder = loader.SlotFeeder(rau, d, fdir, D, W, H)
    assert rau.resizes == [TB] and feeder.n == TB              # switched once, when the feeder was made
    feeder.next()
    ref = make()
    for slot, has_labels, feats, tokens, lens in rau.uploads:
        f, x, xl, a, q = ref.next_batch_feat(fdir, D, W, H)
        assert not has_labels and feats.shape == (TB, D, W * H)
        np.testing.assert_array_equal(feats, f.reshape(TB, D, W * H))
        np.testing.assert_array_equal(tokens, x)
        np.testing.assert_array_equal(lens, xl)
    assert [u[0] for u in rau.uploads] == [0, 1] and rau.resizes == [TB]
    rau.set_batch_size(CAP)                                    # back to training: the feeder's slots are gone
    with pytest.raises(RuntimeError):
        feeder.next()
    big = loader.DataClass(d.qs, d.img_names, CAP + 1, "test")
    with pytest.raises(ValueError):
        loader.SlotFeeder(rau, big, fdir, D, W, H)             # above the capacity
