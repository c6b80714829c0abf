"""Region counts, the parts that need no device: the ABI's statement of them, the numpy gather, and the
identities of the per-sample reference (tests/regions_ref.py) the GPU tests are measured against."""
import os
import re

import numpy as np
import pytest

import oracle
from tests import regions_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points_and_keeps_abi_5():
    text = open(os.path.join(ROOT, "include", "rau.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert re.search(r"int rau_set_regions\(rau_ctx\* ctx, int slot, const int32_t\* n ?\);", flat)
    assert "int rau_batch_regions(rau_ctx* ctx, int* has);" in flat
    m = re.search(r"int rau_multimodal_forward_regions\(([^)]*)\)", flat)
    assert m and "const int32_t* regions_dev" in m.group(1)
    assert re.search(r"#define RAU_ABI_VERSION 5\b", text)


def test_ctypes_table_lists_them():
    from rau_vqa_amd import _lib
    for name in ("rau_set_regions", "rau_batch_regions", "rau_multimodal_forward_regions"):
        assert name in _lib._SIGS
    # rau_multimodal_forward plus one pointer
    assert len(_lib._SIGS["rau_multimodal_forward_regions"][1]) == len(_lib._SIGS["rau_multimodal_forward"][1]) + 1


def test_regions_of_gathers_per_image_counts():
    from rau_vqa_amd.model import regions_of
    n_image = np.array([36, 10, 100], np.int64)
    image_of = np.array([2, 0, 0, 1, 2], np.int32)
    got = regions_of(n_image, image_of)
    assert got.dtype == np.int32 and got.flags.c_contiguous
    assert got.tolist() == [100, 36, 36, 10, 100]
    assert regions_of(n_image, np.zeros(0, np.int32)).shape == (0,)
    for bad in ([3], [-1]):
        with pytest.raises(ValueError):
            regions_of(n_image, np.array(bad, np.int32))
    with pytest.raises(ValueError):
        regions_of(np.ones((2, 2), np.int32), image_of)


def test_loader_feed_passes_a_dict_batch_and_its_regions():
    from rau_vqa_amd import loader

    class Rec:
        def __init__(self):
            self.calls = []

        def set_batch(self, **kw):
            self.calls.append(("set_batch", kw))

        def set_regions(self, n):
            self.calls.append(("set_regions", n))

    r = Rec()
    batch = {"feats": 1, "tokens": 2, "lens": 3, "labels": 4, "regions": [5, 6], "qids": [7, 8]}
    assert loader.feed(r, batch) == [7, 8]
    assert r.calls == [("set_batch", {"feats": 1, "tokens": 2, "lens": 3, "labels": 4, "regions": [5, 6]})]
    r = Rec()
    loader.feed(r, batch, regions=[1, 1])          # the argument replaces the key
    assert r.calls == [("set_batch", {"feats": 1, "tokens": 2, "lens": 3, "labels": 4}), ("set_regions", [1, 1])]


def test_dataclass_reports_per_sample_counts_of_the_batch():
    from rau_vqa_amd.loader import DataClass, QuestionSet
    N = 6
    qs = QuestionSet(question=np.ones((N, 3), np.int32), lengths_q=np.full(N, 3, np.int32),
                     img_list=np.array([1, 3, 3, 2, 1, 2]), question_id=np.arange(N),
                     answers=np.ones(N, np.int32), img_regions=np.array([36, 10, 100]))
    d = DataClass(qs, ["a", "b", "c"], batch_size=4)
    d._take(np.array([0, 1, 2, 3]))
    assert d.last_regions.dtype == np.int32 and d.last_regions.tolist() == [36, 100, 100, 10]
    qs.img_regions = None
    d._take(np.array([0, 1, 2, 3]))
    assert d.last_regions is None


# ---- the reference's identities (fp64, SMALL at B = 4, seed 7)
SH = util.shapes(util.SMALL, B=4)
COUNTS = np.array([12, 7, 3, 1])


@pytest.fixture(scope="module")
def problem():
    batch, params, masks = util.make_problem(SH, seed=7, scale=0.5)
    hop_w = np.full(SH.H, float(SH.H), np.float32)
    full = oracle.step(SH, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks, hop_w,
                       dtype=np.float64)
    return batch, params, masks, hop_w, full


def test_all_counts_equal_to_S_is_the_batched_oracle(problem):
    batch, params, masks, hop_w, full = problem
    ref = regions_ref.step(SH, params, batch, masks, hop_w, np.full(SH.B, SH.S))
    for k in util.OUT_KEYS + util.GRAD_KEYS:
        assert util.rel_err(ref[k], full[k]) <= 1e-12, k
    assert np.array_equal(ref["argmax"], full["argmax"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_masked_positions_get_exactly_zero_attention(problem, dtype):
    batch, params, masks, hop_w, full = problem
    ref = regions_ref.step(SH, params, batch, masks, hop_w, COUNTS, dtype=dtype)
    att = ref["att"]
    for b, n in enumerate(COUNTS):
        assert np.all(att[:, b, n:] == 0), b
        assert np.all(att[:, b, :n] > 0), b
    np.testing.assert_allclose(att.sum(axis=2), 1.0, rtol=0, atol=1e-6 if dtype == np.float32 else 1e-14)
    for k in util.OUT_KEYS + util.GRAD_KEYS:
        assert np.all(np.isfinite(ref[k])), k
    if dtype == np.float64:
        # the counts matter: a device that ignores them misses the 1e-4 bar by orders of magnitude
        moved = [util.rel_err(ref["logits"][:, b], full["logits"][:, b]) for b in range(1, SH.B)]
        assert max(moved) > 1e-2, moved
        assert util.rel_err(ref["logits"][:, 0], full["logits"][:, 0]) <= 1e-12    # count = S: untouched
        # attbymemory's weight rows and bias of positions nobody attends to get no gradient
        top = 9
        g = regions_ref.step(SH, params, batch, masks, hop_w, np.minimum(COUNTS, top))["g_mult"]
        sl = regions_ref.bias_slice(SH)
        gw = g[sl.start - SH.S * SH.R:sl.start].reshape(SH.S, SH.R)
        assert np.all(gw[top:] == 0) and np.all(g[sl][top:] == 0)
        assert np.all(np.abs(gw[:top]).max(axis=1) > 0)
