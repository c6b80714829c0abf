"""Host side of the per-image feature-map gradient (RAU_FEAT_GRAD_IMAGES): the declarations in the header, the
ctypes table and the Lua binding, the null-argument answers, the sample lists the batch code builds
(rau_image_lists) and the numpy statement of the device's arithmetic (joint.image_hop_sum).  No device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rau_vqa_amd import _lib as L
from rau_vqa_amd import joint
from tests import featgrad_ref
from tests.test_abi import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rau_feat_grad_rows", "rau_set_batch_dev_images", "rau_image_lists")
MODES = {"OFF": 0, "SAMPLES": 1, "IMAGES": 2}
INVALID = -1


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_header_ctypes_and_lua_agree_on_the_new_calls_and_the_mode_names():
    header, lua = read("include", "rau.h"), read("bindings", "rau.lua")
    assert re.search(r"#define RAU_ABI_VERSION 5\b", header)          # the interface only grew
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    want, got = _prototypes(header), _prototypes(cdef)
    for name in NEW:
        assert name in want and got.get(name) == want[name], name
        assert name in L._SIGS
        assert len(L._SIGS[name][1]) == want[name].count(",") + 1, name    # one ctypes argument per parameter
    for name, value in MODES.items():
        assert re.search(r"#define RAU_FEAT_GRAD_%s %d\b" % (name, value), header), name
        assert getattr(L, "FEAT_GRAD_" + name) == value
    assert re.search(r"RAU\.FEAT_GRAD_OFF, RAU\.FEAT_GRAD_SAMPLES, RAU\.FEAT_GRAD_IMAGES = 0, 1, 2\b", lua)
    for wrapper in ("function RAU:wantFeatureGrad(on, perImage)", "function RAU:featureGradRows()",
                    "function RAU:setBatchDevImages(table_dev, n_images, image_of, x, x_len, y)"):
        assert wrapper in lua, wrapper
    for call in ("C.rau_feat_grad_rows(", "C.rau_set_batch_dev_images("):
        assert call in lua, call


def test_new_entry_points_answer_a_null_ctx():
    lib = L.lib()
    rows = C.c_int32(0)
    idx = np.zeros(1, np.int32)
    for rc in (lib.rau_feat_grad_rows(None, C.byref(rows)),
               lib.rau_set_batch_dev_images(None, None, 1, idx.ctypes.data, idx.ctypes.data, idx.ctypes.data, None),
               lib.rau_set_feat_grad(None, 2)):
        assert rc == INVALID and b"null" in lib.rau_last_error()
    assert lib.rau_image_lists(1, 1, None, None, None) == INVALID and b"null" in lib.rau_last_error()


def image_lists(n_images, image_of):
    image_of = np.ascontiguousarray(image_of, np.int32)
    guard = 4                                   # words on either side of both outputs that must stay untouched
    start = np.full(n_images + 1 + 2 * guard, -7, np.int32)
    samples = np.full(image_of.size + 2 * guard, -7, np.int32)
    rc = L.lib().rau_image_lists(image_of.size, n_images, image_of.ctypes.data, start[guard:].ctypes.data,
                                 samples[guard:].ctypes.data)
    for a in (start, samples):
        assert np.all(a[:guard] == -7) and np.all(a[-guard:] == -7)
    return rc, start[guard:-guard], samples[guard:-guard]


@pytest.mark.parametrize("n_images,image_of", [
    (4, [2, 0, 2, 2, 0, 3]),            # non-monotone, fan-out 3, image 1 without a sample
    (6, list(range(6))),                # the identity
    (1, [0, 0, 0, 0, 0]),               # every sample on one image
    (3, [2, 2, 2, 2]),                  # ... on the last one: leading images empty
    (1, [0]),                           # n = 1
], ids=["fanout_unnamed", "identity", "one_image", "last_image", "n1"])
def test_image_lists(n_images, image_of):
    rc, start, samples = image_lists(n_images, image_of)
    n = len(image_of)
    assert rc == 0
    assert start[0] == 0 and start[n_images] == n and np.all(np.diff(start) >= 0)
    assert sorted(samples.tolist()) == list(range(n))                 # every sample exactly once
    for i in range(n_images):
        mine = samples[start[i]:start[i + 1]]
        assert np.all(np.diff(mine) > 0)                              # ascending within the image
        assert mine.tolist() == [b for b in range(n) if image_of[b] == i]


@pytest.mark.parametrize("n_images,image_of", [(4, [0, 4]), (4, [-1, 0]), (3, [0, 1]), (0, [0])],
                         ids=["past_the_table", "negative", "more_images_than_samples", "no_image"])
def test_image_lists_refuse_bad_arguments(n_images, image_of):
    rc, start, samples = image_lists(n_images, image_of)
    assert rc == INVALID and b"rau_image_lists" in L.lib().rau_last_error()
    assert np.all(start == -7) and np.all(samples == -7)              # nothing was written


# ------------------------------------------------------------------------------------------ image_hop_sum
HA, N_S, D, S, SP, P = 3, 6, 5, 9, 12, 0.3
IMAGE_OF = np.array([2, 0, 2, 2, 0, 3], np.int32)


def random_terms(seed=3):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(HA, N_S, D, SP)).astype(np.float32)
    keep = (rng.random(size=(HA, N_S, D, S)) >= P).astype(np.uint8)
    return G, keep


@pytest.mark.parametrize("masked", [True, False])
def test_image_hop_sum_against_an_fp64_sum(masked):
    G, keep = random_terms()
    keep = keep if masked else None
    got = joint.image_hop_sum(G, keep, P, S, SP, IMAGE_OF, 4)
    assert got.dtype == np.float32 and got.shape == (4, D, SP)
    s_x = 1.0 / (1.0 - P) if masked else 1.0
    terms = G[..., :S].astype(np.float64) * s_x * (keep if masked else 1.0)
    ref = np.zeros((4, D, S))
    mag = np.zeros((4, D, S))
    for b in range(N_S):
        ref[IMAGE_OF[b]] += terms[:, b].sum(0)
        mag[IMAGE_OF[b]] += np.abs(terms[:, b]).sum(0)
    # HA * fan-out <= 9 terms, each rounded once (2^-24 relative) and each of the 8 additions once more: below
    # 2 * 9 * 2^-24 of the sum of magnitudes, taken elementwise
    assert np.all(np.abs(got[..., :S] - ref) <= 18 * 2.0 ** -24 * mag + 1e-45)
    assert not got[1].any() and not got[..., S:].any()                # the unnamed image, the pad columns: exact zeros
    assert got[0].any() and got[2].any() and got[3].any()


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("order", [None, [2, 0, 1]])
def test_image_hop_sum_with_the_identity_table_is_masked_hop_sum(masked, order):
    G, keep = random_terms(seed=4)
    keep = keep if masked else None
    a = joint.image_hop_sum(G, keep, P, S, SP, np.arange(N_S), N_S, order=order)
    b = featgrad_ref.masked_hop_sum(G, keep, P, S, SP, order=order)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_image_hop_sum_checks_the_index():
    G, keep = random_terms()
    with pytest.raises(ValueError):
        joint.image_hop_sum(G, keep, P, S, SP, IMAGE_OF, 3)
    with pytest.raises(ValueError):
        joint.image_hop_sum(G, keep, P, S, SP, IMAGE_OF[:5], 4)
