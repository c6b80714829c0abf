"""Packed region features on the GPU (rau_set_batch_packed, rau_set_batch_async_packed, rau_bank_put_packed).

The contract is feat16.unpack_regions: a packed batch gives, bit for bit, what the dense batch
unpack_regions(rows, counts, S) followed by set_regions gives.  Every comparison is np.array_equal: the feature only
moves bytes (the f32 -> narrower bank form narrows with the bits of bank_put).

1. kernel     the bytes behind rau_batch_feats at pitch Sp, pad columns included, after a buffer full of junk;
2. bank       bank_put_packed + bank_get; f32 rows narrowed into the four narrower banks; other rows untouched;
3. identity   every output and gradient of a packed step == the dense step with set_regions, on every way in;
4. lifetime   of a packed batch and its counts in the two slots;
5. launches   a dense step launches what it did; a packed step adds exactly the unpack launch;
6. errors     leave the previous batch resident and its results reproducible.
"""
import ctypes as C

import numpy as np
import pytest

from rau_vqa_amd import feat16
from tests import util
from tests.test_gpu_att_variants import SEVEN
from tests.test_gpu_regions import (BOXES, INVALID, STATE, assert_masked, assert_same_bits, counts_of, differs,
                                    hop_weights, make, results, set_mode)

pytestmark = pytest.mark.gpu

TYPES = ("f32", "f16", "bf16", "e4m3", "e5m2")
BIG = dict(B=2, T=4, V=9, E=4, Rq=4, D=2048, S=36, M=4, A=4, R=4, K=4, H=1)
# The unpack tile is 64 channels x 64 positions of one map, moved as quads of 4 positions (csrc/packed.h).
# Counts on both sides of each edge:
#   position tile edge 64   boxes: 57 and 64 end in the first tile, 99 and 100 in the second; 1, 10, 36 far below
#   quad edges              boxes: 10, 99, 57, 1 end inside a quad, 100, 36, 64 on one; seven: 49 = S in the pad quad
#                           (Sp = 52), 48 the last full quad, 1, 17, 30, 5 inside; edge: 4 = S = one quad, 1, 2, 3
#   channel tile edges      D = 24 and 4 (one partial tile), 68 (64 + 4), 132 (128 + 4), 2048 (32 full tiles)
SHAPES = {
    "boxes": (BOXES, [100, 10, 99, 36, 1, 57, 64, 100]),
    "seven": (SEVEN, [49, 48, 1, 17, 30, 5]),
    "edge": (util.EDGE, [4, 1, 3, 2, 4]),
    "boxes68": (dict(BOXES, D=68), [100, 10, 99, 36, 1, 57, 64, 100]),
    "boxes132": (dict(BOXES, D=132), [100, 10, 99, 36, 1, 57, 64, 100]),
    "big": (BIG, [36, 1]),
    # the fused attention family's bound: 15 position tiles, the last one 4 wide; counts on tile edges (257, 513),
    # inside the last tile (899, 900) and far below it
    "boxes900": (dict(BOXES, S=900), [900, 10, 899, 257, 1, 513, 770, 900]),
}


def codes_of(x, ft):
    """f32 values as elements of feat type ft (fp8 and bf16 as their bit patterns)."""
    if ft in ("e4m3", "e5m2"):
        return feat16.fp8_bits(x, ft)
    if ft == "bf16":
        return feat16.bf16_bits(x)
    return x.astype(feat16.dtype_of(ft))


def pack(maps, counts):
    """dense maps [N, D, S] -> rows [sum(counts), D]: the first counts[i] positions of map i, one row each."""
    return np.ascontiguousarray(np.concatenate([maps[i, :, :c].T for i, c in enumerate(counts)]))


def feats_bytes(m, n_maps, dtype):
    """The first n_maps maps behind rau_batch_feats as [n_maps, D, Sp] of dtype."""
    c = m.cfg
    Sp = (c.S + 3) // 4 * 4
    p = C.c_void_p()
    assert m._lib.rau_batch_feats(m._h, C.byref(p)) == 0
    out = np.empty((n_maps, c.D, Sp), dtype)
    assert m._lib.rau_dev_download(m._h, out.ctypes.data, p, out.nbytes) == 0
    return out


def poison(m):
    """Fill the whole resident feature buffer ([B, D, Sp] floats) with junk."""
    c = m.cfg
    p = C.c_void_p()
    assert m._lib.rau_batch_feats(m._h, C.byref(p)) == 0
    junk = np.full(c.B * c.D * ((c.S + 3) // 4 * 4) * 4, 0xAB, np.uint8)
    assert m._lib.rau_dev_upload(m._h, p, junk.ctypes.data, junk.nbytes) == 0


def at_pitch(dense, Sp):
    out = np.zeros(dense.shape[:2] + (Sp,), dense.dtype)
    out[:, :, :dense.shape[2]] = dense
    return out


# ---------------------------------------------------------------- 1. kernel
KERNEL_CASES = [("boxes", ft) for ft in TYPES] + [(n, ft) for n in ("seven", "edge", "boxes68", "boxes132", "big",
                                                                    "boxes900") for ft in ("f32", "e4m3")]


@pytest.mark.parametrize("name,ft", KERNEL_CASES, ids=[f"{n}-{ft}" for n, ft in KERNEL_CASES])
def test_unpacked_bytes_equal_the_contract_pad_columns_included(name, ft):
    """Edges: see the table at SHAPES (position tile 64, quads of 4, channel tiles of 64)."""
    dims, counts = SHAPES[name]
    counts = np.array(counts, np.int32)
    m, sh, batch, params, masks = make(dims)
    Sp = (sh.S + 3) // 4 * 4
    rng = np.random.default_rng(3)
    src = codes_of(rng.uniform(-4, 4, (sh.B, sh.D, sh.S)).astype(np.float32), ft)
    src[src == 0] = 1                                           # no element of a row is all zero bits
    rows = pack(src, counts)
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    # a dense batch of another element size first, then junk in every byte of the buffer, pad columns too
    other = "e4m3" if ft == "f32" else "f32"
    m.set_batch(codes_of(np.full((sh.B, sh.D, sh.S), 1.5, np.float32), other), *tok, feat_type=other)
    poison(m)
    m.set_batch_packed(rows, counts, *tok, feat_type=ft)
    want = at_pitch(feat16.unpack_regions(rows, counts, sh.S), Sp)
    got = feats_bytes(m, sh.B, rows.dtype)
    assert m.batch_feat_type() == ft and m.batch_regions() and m.batch_images() == 0
    m.close()
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(want.dtype) != want)[:8]
    for i, c in enumerate(counts):                              # the contract itself, spelt out
        assert np.array_equal(got[i, :, :c], src[i, :, :c]) and not got[i, :, c:].view(np.uint8).any()


def test_an_image_table_is_unpacked_map_by_map():
    dims, _ = SHAPES["seven"]
    m, sh, batch, params, masks = make(dims)
    counts = np.array([30, 49, 1, 48], np.int32)
    image_of = np.array([3, 0, 0, 2, 1, 3], np.int32)
    src = codes_of(np.random.default_rng(4).uniform(1, 2, (4, sh.D, sh.S)).astype(np.float32), "f16")
    rows = pack(src, counts)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    poison(m)
    m.set_batch_packed(rows, counts, batch["tokens"], batch["lens"], batch["labels"], image_of=image_of)
    got = feats_bytes(m, 4, np.float16)
    assert m.batch_images() == 4 and m.batch_feat_type() == "f16" and m.batch_regions()
    m.close()
    assert got.tobytes() == at_pitch(feat16.unpack_regions(rows, counts, sh.S), 52).tobytes()


# ---------------------------------------------------------------- 2. bank
@pytest.mark.parametrize("name", ["boxes", "seven"])
def test_bank_put_packed_then_get_is_the_contract(name):
    dims, counts = SHAPES[name]
    counts = np.array(counts, np.int32)
    m, sh, batch, params, masks = make(dims)
    N, cap = counts.size, counts.size + 4
    rng = np.random.default_rng(8)
    for ft in TYPES:
        src = codes_of(rng.uniform(-4, 4, (N, sh.D, sh.S)).astype(np.float32), ft)
        src[src == 0] = 1
        fence = codes_of(np.full((cap, sh.D, sh.S), 3.0, np.float32), ft)
        rows = pack(src, counts)
        m.bank_create(cap, ft)
        m.bank_put(0, fence, feat_type=ft)
        m.bank_put_packed(2, rows, counts, feat_type=ft)
        got = m.bank_get(0, cap)
        assert m.bank_info()["rows_filled"] == cap
        m.bank_destroy()
        assert got[2:2 + N].tobytes() == feat16.unpack_regions(rows, counts, sh.S).tobytes(), ft
        assert got[:2].tobytes() == fence[:2].tobytes() and got[2 + N:].tobytes() == fence[2 + N:].tobytes(), ft
    m.close()


def test_bank_put_packed_in_more_than_one_chunk():
    """The put goes through 32 MiB of pinned staging in chunks of whole maps: 140 maps of 30..36 rows at D = 2048 are
    more than 4200 rows of 8 KiB, so a second chunk starts inside the range, with offsets that restart at 0."""
    m, sh, batch, params, masks = make(BIG)
    rng = np.random.default_rng(12)
    counts = rng.integers(30, sh.S + 1, 140).astype(np.int32)
    counts[[0, 70, 139]] = [sh.S, 30, sh.S]
    rows = rng.integers(1, 2 ** 31, (int(counts.sum()), sh.D), dtype=np.int64).astype(np.uint32).view(np.float32)
    assert rows.nbytes > 32 << 20
    m.bank_create(142)
    m.bank_put_packed(1, rows, counts)
    got = m.bank_get(0, 142)
    m.close()
    assert got[1:141].tobytes() == feat16.unpack_regions(rows, counts, sh.S).tobytes()
    assert not got[0].view(np.uint32).any() and not got[141].view(np.uint32).any()


@pytest.mark.parametrize("name", ["boxes", "seven"])
def test_f32_rows_are_narrowed_with_the_bits_of_bank_put(name):
    from tests.test_gpu_bank import crafted
    from tests.test_gpu_fp8 import values_and_codes
    dims, counts = SHAPES[name]
    counts = np.array(counts, np.int32)
    m, sh, batch, params, masks = make(dims)
    N = counts.size
    rng = np.random.default_rng(9)
    for ft in ("f16", "bf16", "e4m3", "e5m2"):
        n = int(counts.sum()) * sh.D
        bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)          # every exponent, inf and NaN too
        vals = bits.view(np.float32).copy()
        vals[::3] = (rng.standard_normal(vals[::3].size) * 10.0 ** rng.uniform(-9, 5, vals[::3].size)).astype(np.float32)
        if ft in ("f16", "bf16"):
            # their contract is stated for finite inputs and the quiet NaN: subnormals and overflow included
            vals[~np.isfinite(vals)] = 1.0
            cases = np.concatenate([crafted(), np.array([np.inf, -np.inf, np.nan], np.float32)])
        else:
            cases = values_and_codes(ft)[0]                     # subnormal, saturating and NaN inputs
        vals[:cases.size] = cases
        rows = vals.reshape(-1, sh.D)
        wide = feat16.unpack_regions(rows, counts, sh.S)
        want = np.empty(wide.shape, feat16.dtype_of(ft))
        with np.errstate(over="ignore", invalid="ignore"):
            feat16.store(want, wide, ft)
        m.bank_create(N, ft)
        m.bank_put_packed(0, rows, counts)
        got = m.bank_get(0, N)
        m.bank_destroy()
        nan = np.isnan(wide)
        assert nan.any() and np.isinf(wide).any()
        u = np.uint8 if ft in ("e4m3", "e5m2") else np.uint16
        bad = np.flatnonzero((got.view(u) != want.view(u)).ravel() & ~nan.ravel())
        assert bad.size == 0, (ft, bad.size, [(float(wide.ravel()[i]), hex(got.view(u).ravel()[i]),
                                               hex(want.view(u).ravel()[i])) for i in bad[:8]])
        assert np.all(np.isnan(feat16.widen(got.view(u)[nan] if ft != "f16" else got[nan], ft)))
        for i, c in enumerate(counts):
            assert not got[i, :, c:].view(u).any(), (ft, i)     # +0 behind the count
    m.close()


# ---------------------------------------------------------------- 3. step identity
IDENT = [("boxes", "f32"), ("seven", "bf16"), ("boxes900", "f32")]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name,ft", IDENT, ids=[n for n, _ in IDENT])
def test_a_packed_step_is_the_dense_step_with_set_regions(name, ft, mode, dtype):
    from rau_vqa_amd.model import regions_of
    dims, counts = SHAPES[name]
    counts = np.array(counts, np.int32)
    m, sh, batch, params, masks = make(dims, dtype=dtype)
    hop_w = hop_weights(sh)
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    src = codes_of(batch["feats"], ft)
    rows = pack(src, counts)
    dense = feat16.unpack_regions(rows, counts, sh.S)
    set_mode(m, mode, masks)
    # ---- plain batch
    m.set_batch(dense, *tok, feat_type=ft, regions=counts)
    ref = results(m, hop_w)
    assert_masked(ref["att"], counts)
    m.set_batch(src, *tok, feat_type=ft)
    assert differs(ref, results(m, hop_w))                      # the counts and the zeros matter
    m.set_batch_packed(rows, counts, *tok, feat_type=ft)
    assert m.batch_regions() and m.batch_images() == 0 and m.batch_feat_type() == ft
    got = results(m, hop_w)
    assert_same_bits(ref, got)
    assert_masked(got["att"], counts)
    # ---- the slot form, rows passed, and rows written in place into the staging
    m.set_batch_async(1, rows, *tok, feat_type=ft, packed_counts=counts)
    m.use_batch(1)
    assert m.batch_regions()
    assert_same_bits(ref, results(m, hop_w))
    st = m.batch_slot(0, ft)
    st["feats"].reshape(-1)[:rows.size] = rows.ravel()
    st["tokens"][...], st["lens"][...], st["labels"][...] = tok
    m.set_batch_async(0, feat_type=ft, packed_counts=counts)
    m.use_batch(0)
    assert_same_bits(ref, results(m, hop_w))
    if mode == "train":
        m.set_batch_packed(rows, counts, *tok, feat_type=ft)
        assert_same_bits(ref, results(m, hop_w, graph=True))
        m.set_batch_packed(rows, counts, *tok, feat_type=ft)    # a replay
        assert_same_bits(ref, results(m, hop_w, graph=True))
    # ---- image table with repeats: counts per image (an evaluate-mode table forward has no backward)
    N = sh.B - 2
    image_of = ((np.arange(sh.B) * 5 + 1) % N).astype(np.int32)   # every image, two of them twice
    n_img = counts[:N]
    trows = pack(src[:N], n_img)
    bwd = mode == "train"
    m.set_batch(dense[:N], *tok, feat_type=ft, image_of=image_of, regions=n_img)
    tref = results(m, hop_w, backward=bwd)
    m.set_batch_packed(trows, n_img, *tok, feat_type=ft, image_of=image_of)
    assert m.batch_images() == N and m.batch_regions()
    got = results(m, hop_w, backward=bwd)
    assert_same_bits(tref, got)
    assert_masked(got["att"], regions_of(n_img, image_of))
    m.set_batch_async(1, trows, *tok, feat_type=ft, image_of=image_of, packed_counts=n_img)
    m.use_batch(1)
    assert_same_bits(tref, results(m, hop_w, backward=bwd))
    # ---- bank batch out of a bank filled by bank_put_packed
    m.bank_create(N + 3, ft)
    m.bank_put_packed(2, trows, n_img, feat_type=ft)
    m.set_batch(None, *tok, bank_rows=np.arange(2, 2 + N), image_of=image_of, regions=n_img)
    assert_same_bits(tref, results(m, hop_w, backward=bwd))
    m.close()


# ---------------------------------------------------------------- 4. lifetime and slots
def test_lifetime_of_a_packed_batch_in_the_two_slots():
    from rau_vqa_amd._lib import RauError
    dims, counts = SHAPES["seven"]
    counts = np.array(counts, np.int32)
    m, sh, batch, params, masks = make(dims)
    hop_w = hop_weights(sh)
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    rows = pack(batch["feats"], counts)
    dense = feat16.unpack_regions(rows, counts, sh.S)
    other = np.ascontiguousarray(batch["feats"][::-1])
    m.evaluate()
    m.set_batch(dense, *tok, regions=counts)
    counted = results(m, hop_w)
    m.set_batch(other, *tok)
    free = results(m, hop_w)
    assert differs(free, counted)
    # a packed batch goes into slot 1 while slot 0's step runs
    m.zero_grads()
    m.forward()
    m.set_batch_async(1, rows, *tok, packed_counts=counts)
    m.backward(hop_w)
    assert not m.batch_regions()                                # the resident batch is still slot 0's
    assert np.array_equal(m.outputs()["logits"], free["logits"])
    m.use_batch(1)
    assert m.batch_regions() and m.batch_images() == 0 and m.batch_feat_type() == "f32"
    assert_same_bits(counted, results(m, hop_w))
    m.set_regions(counts[::-1].copy())                          # a later set_regions replaces the counts
    assert differs(counted, results(m, hop_w))
    m.set_batch_async(0, rows, *tok, packed_counts=counts)      # the other slot: slot 1 keeps its batch
    assert m.batch_regions()
    m.use_batch(0)
    assert_same_bits(counted, results(m, hop_w))
    m.set_batch_async(1, other, *tok)                           # a dense upload into the slot drops the counts
    m.use_batch(1)
    assert not m.batch_regions()
    assert_same_bits(free, results(m, hop_w))
    m.use_batch(0)                                              # slot 0 still holds its packed batch
    assert m.batch_regions()
    assert_same_bits(counted, results(m, hop_w))
    m.set_batch(other, *tok)                                    # the synchronous form drops them too
    assert not m.batch_regions()
    assert_same_bits(free, results(m, hop_w))
    m.set_batch_packed(rows, counts, *tok)
    m.set_batch_size(sh.B - 1)                                  # clears the batch
    assert not m.batch_regions()
    with pytest.raises(RauError):
        m.forward()
    m.set_batch_size(sh.B)
    m.evaluate()
    m.set_batch_packed(rows, counts, *tok)
    assert_same_bits(counted, results(m, hop_w))
    m.close()


# ---------------------------------------------------------------- 5. nothing changed for others
def test_a_dense_step_launches_what_it_did_and_a_packed_step_adds_the_unpack():
    from tests.test_gpu_regions import PARENT_LAUNCHES
    from tests.test_gpu_regions import SHAPES as REGION_SHAPES
    dims, scale = REGION_SHAPES["small"]
    counts = counts_of("small")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    rows = pack(batch["feats"], counts)

    def listing(upload):
        m.prof_reset()
        m.prof_enable()
        set_mode(m, "train", masks)
        upload()
        out = results(m, hop_w)
        m.sync()
        got = {k: v["launches"] for k, v in m.prof().items() if v["launches"]}
        m.prof_enable(False)
        return got, out
    dense, _ = listing(lambda: m.set_batch(batch["feats"], *tok))
    assert dense == PARENT_LAUNCHES["small"]                    # recorded before the unpack class existed
    counted, ref = listing(lambda: m.set_batch(feat16.unpack_regions(rows, counts, sh.S), *tok, regions=counts))
    packed, got = listing(lambda: m.set_batch_packed(rows, counts, *tok))
    m.close()
    assert "unpack_regions" not in counted
    assert packed == dict(counted, unpack_regions=1)
    assert_same_bits(ref, got)


# ---------------------------------------------------------------- 6. errors
def test_errors_leave_the_previous_batch_resident():
    dims, counts = SHAPES["seven"]
    counts = np.array(counts, np.int32)
    m, sh, batch, params, masks = make(dims)
    hop_w = hop_weights(sh)
    tokens, lens, labels = batch["tokens"], batch["lens"], batch["labels"]
    rows = pack(batch["feats"], counts)
    lib, h = m._lib, m._h
    F32 = 0

    def p(a):
        return None if a is None else a.ctypes.data

    def sync(n=None, rows_=rows, ft=F32, n_maps=sh.B, image_of=None, tok=tokens):
        n = counts if n is None else np.ascontiguousarray(n, np.int32)
        return lib.rau_set_batch_packed(h, p(rows_), ft, n_maps, p(n), p(image_of), p(tok), p(lens), p(labels))

    def slot(s, n=None, ft=F32, n_maps=sh.B, image_of=None):
        n = counts if n is None else np.ascontiguousarray(n, np.int32)
        return lib.rau_set_batch_async_packed(h, s, p(rows), ft, n_maps, p(n), p(image_of), p(tokens), p(lens),
                                              p(labels), 1)
    m.evaluate()
    m.set_batch(batch["feats"], tokens, lens, labels)
    ref = results(m, hop_w)
    zero, over = counts.copy(), counts.copy()
    zero[2], over[4] = 0, sh.S + 1
    ident = np.arange(sh.B, dtype=np.int32)
    bad_of = ident.copy()
    bad_of[3] = sh.B - 1                                        # a table of B - 1 maps has no row B - 1
    bad_tok = tokens.copy()
    bad_tok[0, 0] = sh.V + 1
    for call in (sync, lambda **kw: slot(1, **kw), lambda **kw: slot(0, **kw)):
        assert call(n=zero) == INVALID and call(n=over) == INVALID and call(n=-counts) == INVALID
        assert call(n_maps=0) == INVALID and call(n_maps=sh.B + 1) == INVALID
        assert call(n_maps=sh.B - 1) == INVALID                 # fewer maps than samples without image_of
        assert call(n_maps=sh.B - 1, image_of=bad_of) == INVALID
        assert call(n_maps=sh.B - 1, image_of=-ident) == INVALID
        assert call(ft=3) == INVALID and call(ft=6) == INVALID
    assert sync(rows_=None) == INVALID and sync(tok=bad_tok) == INVALID
    assert lib.rau_set_batch_packed(h, p(rows), F32, sh.B, None, None, p(tokens), p(lens), p(labels)) == INVALID
    assert slot(2) == INVALID
    assert not m.batch_regions() and m.batch_images() == 0
    assert_same_bits(ref, results(m, hop_w))                    # still resident, reproducible
    # the state rule of the slot form: the current batch of a forward whose backward has not run
    m.use_batch(0)
    m.zero_grads()
    m.forward()
    assert slot(0) == STATE
    m.backward(hop_w)
    assert_same_bits(ref, results(m, hop_w))
    # the bank form
    assert lib.rau_bank_put_packed(h, 0, sh.B, p(rows), F32, p(counts)) == STATE          # no bank
    m.bank_create(sh.B + 1, "f16")
    fence = np.full((sh.B + 1, sh.D, sh.S), 2.0, np.float16)
    m.bank_put(0, fence)
    half = rows.astype(np.float16)
    for n in (zero, over):
        assert lib.rau_bank_put_packed(h, 0, sh.B, p(half), 1, p(n)) == INVALID
    assert lib.rau_bank_put_packed(h, 2, sh.B, p(half), 1, p(counts)) == INVALID          # past the capacity
    assert lib.rau_bank_put_packed(h, -1, sh.B, p(half), 1, p(counts)) == INVALID
    assert lib.rau_bank_put_packed(h, 0, 0, p(half), 1, p(counts)) == INVALID
    assert lib.rau_bank_put_packed(h, 0, sh.B, p(half), 2, p(counts)) == INVALID          # bf16 rows, f16 bank
    assert lib.rau_bank_put_packed(h, 0, sh.B, p(half), 3, p(counts)) == INVALID
    assert lib.rau_bank_put_packed(h, 0, sh.B, None, 1, p(counts)) == INVALID
    assert lib.rau_bank_put_packed(h, 0, sh.B, p(half), 1, None) == INVALID
    assert m.bank_get(0, sh.B + 1).tobytes() == fence.tobytes()
    assert_same_bits(ref, results(m, hop_w))
    # the Python layer checks shapes and dtypes before anything reaches the library
    with pytest.raises(ValueError):
        m.set_batch_packed(rows[:-1], counts, tokens, lens, labels)
    with pytest.raises(ValueError):
        m.set_batch_packed(rows, zero, tokens, lens, labels)
    with pytest.raises(ValueError):
        m.set_batch_packed(rows, counts[:-1], tokens, lens, labels)
    with pytest.raises(ValueError):
        m.set_batch_packed(rows.astype(np.uint8), counts, tokens, lens, labels)           # fp8 must be named
    with pytest.raises(ValueError):
        m.bank_put_packed(0, rows[:, :-4], counts)
    with pytest.raises(ValueError):
        m.set_batch_async(1, rows, tokens, lens, labels, packed_counts=counts, regions=counts)
    assert_same_bits(ref, results(m, hop_w))
    m.close()
