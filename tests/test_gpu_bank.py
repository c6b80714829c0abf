"""The device-resident feature bank (rau_bank_*, rau_set_batch_bank / rau_set_batch_async_bank,
include/rau.h): maps put into the bank come back bit for bit, f32 maps put into a 16-bit bank are narrowed
on the device to the bits feat16.store gives on the host, and a batch that names bank rows gives
BIT-IDENTICAL results to the image-table batch of the same maps and to the plain batch -- in evaluate mode,
in train mode with gradients, through the captured step, the upload slots and the module-level calls, and
in a bank larger than 4 GiB.  Bad calls are rejected with nothing enqueued.  The table / plain runs and the
seeded draws are those of tests/test_gpu_shared_images.py."""
import numpy as np
import pytest

import oracle
from rau_vqa_amd import _lib, feat16
from tests import util
from tests.test_gpu_parity import TOL
from tests.test_gpu_shared_images import (D512, SMALL, differing, eval_run, make, table_batch, train_run)

pytestmark = pytest.mark.gpu

INVALID, STATE, NOMEM = -1, -3, -4


def scatter(m, table, capacity, seed, ft=None, put_type=None):
    """A fresh bank of `capacity` maps with `table`'s maps put one by one, out of order, at distinct
    scattered rows; -> rows [N].  put_type: what the maps are handed over as (default: as they are)."""
    m.bank_destroy()                                            # (nothing to do without a bank)
    m.bank_create(capacity, ft or feat16.infer(table, put_type))
    rng = np.random.default_rng(seed)
    rows = rng.permutation(capacity)[:len(table)].astype(np.int32)
    for n in rng.permutation(len(table)):
        m.bank_put(int(rows[n]), table[n:n + 1], feat_type=put_type)
    return rows


def bank_of(tb, rows):
    """The bank batch of a table batch whose maps sit at `rows`."""
    b = {k: v for k, v in tb.items() if k not in ("feats", "feat_type")}
    return dict(b, feats=None, bank_rows=rows)


# ------------------------------------------------------------------------------ put / get
@pytest.mark.parametrize("S", [196, 49])
def test_put_get_round_trip(S):
    d = dict(SMALL, S=S)
    m = make(d)
    rng = np.random.default_rng(S)
    for ft in ("f32", "f16", "bf16"):
        maps = rng.standard_normal((9, d["D"], S)).astype(np.float32)
        maps = maps if ft == "f32" else maps.astype(np.float16) if ft == "f16" else feat16.bf16_bits(maps)
        m.bank_create(11, ft)
        assert m.bank_info() == {"capacity": 11, "feat_type": ft, "rows_filled": 0}
        kw = {"feat_type": "bf16"} if ft == "bf16" else {}
        m.bank_put(7, maps[7:9], **kw)                          # out of order, several maps at once
        m.bank_put(2, maps[0:1], **kw)                          # ... a row that is overwritten below
        m.bank_put(0, maps[0:5], **kw)
        m.bank_put(5, maps[5:7], **kw)
        assert m.bank_info()["rows_filled"] == 9
        got = m.bank_get(0, 9)
        assert got.dtype == maps.dtype and got.tobytes() == maps.tobytes(), ft
        assert m.bank_get(3, 2).tobytes() == maps[3:5].tobytes()
        assert not m.bank_get(9, 2).any()                       # never written: zeros
        m.bank_destroy()
    m.close()


def crafted():
    """f32 values on the fp16 rounding boundaries."""
    f = np.float32
    v = [0.0, -0.0, 1.0, -1.0,
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20,   # ties, both ways
         2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26, 2.0 ** -15, 2.0 ** -24,           # smallest normal, subnormals
         2.0 ** -24 + 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 2.0 ** -26, 2.0 ** -30,
         5 * 2.0 ** -25, 7 * 2.0 ** -25, 1e-40, 1.4e-45,
         65504.0, 65519.0, 65519.996, 65520.0, 65521.0, 65536.0, 1e10, 3.4e38,                           # around the fp16 maximum
         2047.0, 2049.0, 2051.0, 4098.0, 4102.0, 0.1, 1 / 3]
    v = np.array(v, np.float64).astype(f)
    # bf16 ties to even, both ways, and the carry into the exponent
    b = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3FFF8000, 0x3FFFFFFF, 0x7F7F7FFF, 0x00008000,
                  0x00018000], np.uint32).view(f)
    v = np.concatenate([v, b])
    return np.concatenate([v, -v])


def test_device_narrowing_is_feat16_store_bit_for_bit():
    d = SMALL
    per = d["D"] * d["S"]
    n = -(-(1_000_000 + 200) // per)
    rng = np.random.default_rng(77)
    bits = rng.integers(0, 2 ** 32, n * per + 4096, dtype=np.uint64).astype(np.uint32)
    vals = bits.view(np.float32)
    vals = vals[np.isfinite(vals)][:n * per].copy()                   # every exponent, subnormals included
    assert vals.size == n * per and vals.size >= 1_000_000
    # a quarter of them in fp16's own range, where its subnormals and ties live
    vals[::4] = (rng.standard_normal(vals[::4].size) * 10.0 ** rng.uniform(-9, 5, vals[::4].size)).astype(np.float32)
    c = crafted()
    vals[:c.size] = c
    src = vals.reshape(n, d["D"], d["S"])
    m = make(d)
    for ft in ("f16", "bf16"):
        want = np.empty(src.shape, feat16.dtype_of(ft))
        with np.errstate(over="ignore"):
            feat16.store(want, src)
        m.bank_create(n, ft)
        m.bank_put(0, src)                                           # f32 in: narrowed on the device
        got = m.bank_get(0, n)
        bad = np.flatnonzero(got.view(np.uint16).ravel() != want.view(np.uint16).ravel())
        assert bad.size == 0, (ft, bad.size, [(float(vals[i]), hex(got.view(np.uint16).ravel()[i]),
                                               hex(want.view(np.uint16).ravel()[i])) for i in bad[:8]])
        m.bank_destroy()
    # the pairs that are not conversions the bank makes
    lib, one = m._lib, np.clip(src[:1], -1e4, 1e4)
    for bank_ft, src_arr, src_ft in (("f32", one.astype(np.float16), 1), ("f32", feat16.bf16_bits(one), 2),
                                     ("f16", feat16.bf16_bits(one), 2), ("bf16", one.astype(np.float16), 1)):
        m.bank_create(2, bank_ft)
        assert lib.rau_bank_put(m._h, 0, 1, src_arr.ctypes.data, src_ft) == INVALID
        assert m.bank_info()["rows_filled"] == 0
        m.bank_destroy()
    m.close()


# ------------------------------------------------------------------------------ evaluate mode
def eval_three_ways(m, d, N, seed, ft="f32", kind="shuffle", put_f32=False, capacity=40):
    """bank batch == table batch == plain batch, bitwise, on everything eval_run collects."""
    tb, pb = table_batch(d, N, seed, ft, kind)
    if put_f32:   # f32 maps narrowed by the bank against the same maps narrowed on the host
        wide = table_batch(d, N, seed, "f32", kind)[0]["feats"]
        rows = scatter(m, wide, capacity, seed, ft=ft)
    else:
        rows = scatter(m, tb["feats"], capacity, seed, put_type="bf16" if ft == "bf16" else None)
    mc = np.random.default_rng(seed).integers(0, d["K"] + 1, (d["B"], 4)).astype(np.int32)
    got = eval_run(m, bank_of(tb, rows), mc)
    assert m.batch_images() == N and m.batch_feat_type() == ft
    table = eval_run(m, tb, mc)
    plain = eval_run(m, pb, mc)
    assert not differing(got, table), f"bank batch differs from the table batch in {differing(got, table)}"
    assert not differing(got, plain), f"bank batch differs from the plain batch in {differing(got, plain)}"
    return got, pb


def test_eval_d512_three_ways_and_the_oracle():
    """B = 48: N = 16 (also held against the fp64 oracle on the expanded batch, at the suite's bar), N = B
    with a permutation, N = 1."""
    d = D512
    m = make(d)
    params = m.get_params()
    got, pb = eval_three_ways(m, d, 16, seed=140)
    sh = util.shapes(d)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    ref = oracle.step(sh, params, pb["feats"], pb["tokens"], pb["lens"], pb["labels"], None, hop_w, dtype=np.float64)
    errs = {k: util.rel_err(got[k], ref[k]) for k in util.OUT_KEYS}
    print("bank batch vs fp64 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), errs
    assert np.array_equal(got["argmax"], ref["argmax"])
    eval_three_ways(m, d, 48, seed=144, kind="perm", capacity=64)
    eval_three_ways(m, d, 1, seed=145)
    m.close()


def test_eval_d2048_bf16_mode_fp16_bank_filled_with_f32():
    d = dict(D512, D=2048, M=256, A=64)
    m = make(d, "bf16")
    eval_three_ways(m, d, 16, seed=142, ft="f16", put_f32=True)
    m.close()


def test_eval_7x7_maps_bf16_bank():
    d = dict(SMALL, B=80, S=49)
    m = make(d)
    eval_three_ways(m, d, 27, seed=146, ft="bf16", put_f32=True)
    m.close()


def test_table_is_gathered_late_for_a_batch_handed_over_in_train_mode():
    """A bank batch set in train mode carries its index only; an evaluate-mode forward of the same
    resident batch gathers the table then."""
    d = SMALL
    m = make(d)
    tb, pb = table_batch(d, 5, seed=150)
    rows = scatter(m, tb["feats"], 20, 150)
    m.training()
    m.set_batch(**bank_of(tb, rows))
    m.evaluate()
    m.forward()
    got = m.outputs()
    m.set_batch(**pb)
    m.forward()
    assert not differing(got, m.outputs())
    m.close()


# --------------------------------------------------------------------------------- train mode
@pytest.mark.parametrize("S,ft", [(196, "f32"), (49, "f16")])
def test_train_forward_backward_explicit_masks(S, ft):
    d = dict(SMALL, S=S)
    sh = util.shapes(d)
    _, _, masks = util.make_problem(sh, seed=9)
    hop_w = np.array([3.0, 1.0, 3.0], np.float32)
    m = make(d)
    tb, pb = table_batch(d, 5, seed=50, ft=ft)
    rows = scatter(m, tb["feats"], 20, 50)
    got = train_run(m, bank_of(tb, rows), masks, hop_w)
    table = train_run(m, tb, masks, hop_w)
    plain = train_run(m, pb, masks, hop_w)
    assert not differing(got, table), f"train step on a bank batch differs from the table batch in {differing(got, table)}"
    assert not differing(got, plain), f"train step on a bank batch differs from the plain batch in {differing(got, plain)}"
    assert all(np.any(got[g] != 0) for g in ("g_embed", "g_rnn", "g_mult"))
    m.close()


def test_graph_step_replays_with_new_rows_and_a_new_n():
    d = SMALL
    hop_w = np.full(d["H"], 3.0, np.float32)
    mg, me = make(d), make(d)
    lens = np.full(d["B"], d["T"], np.int32)               # one longest length: one graph shape
    mg.bank_create(30, "f32")
    rng = np.random.default_rng(160)
    for it, N in enumerate((5, 5, 9)):                      # new rows, then a new N: both replay
        tb, pb = table_batch(d, N, seed=60 + it)
        tb["lens"] = pb["lens"] = lens
        rows = rng.permutation(30)[:N].astype(np.int32)
        for n in range(N):
            mg.bank_put(int(rows[n]), tb["feats"][n:n + 1])   # between steps: adds and replaces rows
        got = train_run(mg, bank_of(tb, rows), None, hop_w, graph=True, seed_step=(13, it))
        want = train_run(me, pb, None, hop_w, seed_step=(13, it))
        bad = differing(got, want)
        assert not bad, f"replay {it}: captured step on a bank batch differs in {bad}"
    mg.close()
    me.close()


# -------------------------------------------------------------------------------------- slots
def test_slots_bank_and_uploaded_batches_alternate():
    d = dict(SMALL, B=20)
    ma, ms = make(d), make(d)
    ma.evaluate()
    ms.evaluate()
    ma.bank_create(40, "f32")
    stage = ma.batch_slot(0)["feats"]
    stage[...] = 3.0
    for it in range(4):
        slot = it & 1
        tb, pb = table_batch(d, 7, seed=170 + it)
        if slot == 0:                                       # slot 0 holds bank batches, slot 1 uploaded ones
            rows = (np.arange(7) * 5 + it).astype(np.int32)
            ma.bank_put(int(rows[0]), tb["feats"][0:1])
            for n in range(1, 7):
                ma.bank_put(int(rows[n]), tb["feats"][n:n + 1])
            batch = bank_of(tb, rows)
        else:
            batch = dict(pb)
        labels = batch.pop("labels")
        ma.set_batch_async(slot, labels=labels, **batch)
        if it:                                              # the other slot is still the resident batch
            assert ma.batch_images() == (0 if slot == 0 else 7)
        ma.use_batch(slot)
        assert ma.batch_images() == (7 if slot == 0 else 0)
        ma.forward()
        got = ma.outputs()
        ms.set_batch(**pb)
        ms.forward()
        bad = differing(got, ms.outputs())
        assert not bad, f"step {it} (slot {slot}) differs from the synchronous plain batch in {bad}"
    ma.sync()
    assert (ma.batch_slot(0)["feats"] == 3.0).all()         # a bank batch never touches the feature staging
    ma.close()
    ms.close()


# -------------------------------------------------------------------------------- module level
def test_multimodal_forward_on_the_resident_bank_batch():
    import torch
    from rau_vqa_amd import modules
    d = dict(SMALL, H=2)
    m = make(d)
    m.training()
    m.set_dropout_seed(8, 1)
    c = m.cfg
    q = torch.as_tensor(np.random.default_rng(2).uniform(-1, 1, (c.B, c.Q)).astype(np.float32)).cuda()
    tb, pb = table_batch(d, 4, seed=80)
    rows = scatter(m, tb["feats"], 10, 80)

    def clone_run(batch):
        m.set_batch(**batch)
        outs = []
        for h in range(c.H):
            fwd = modules.MultimodalClone(m, h).forward(q, None, None, None)   # X = NULL: the resident batch
            m.sync()
            outs += [x.cpu().numpy().copy() for x in fwd]
        return outs
    got, want = clone_run(bank_of(tb, rows)), clone_run(pb)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a, b)]
    assert not bad, f"module-level outputs {bad} differ"
    m.close()


# ------------------------------------------------------------------------------ beyond 4 GiB
def test_bank_beyond_4_gib():
    """D = 2048, fp16: a map is 802 816 bytes, so row 5 350 starts beyond 2^32.  Only rows 0, 1 and
    5 349 .. 5 499 are written; a batch drawn from both ends equals the table batch of the same maps, in
    evaluate mode (table gather) and in train mode (gather with the composed index)."""
    d = dict(B=16, T=9, V=300, E=200, Rq=64, D=2048, S=196, M=64, A=32, R=64, K=1000, H=2)
    m = make(d)
    m.bank_create(5500, "f16")
    assert 5350 * d["D"] * d["S"] * 2 > 2 ** 32
    rng = np.random.default_rng(190)
    base = rng.standard_normal((d["D"], d["S"])).astype(np.float32)
    hi = np.stack([(base * (1 + 0.01 * (r % 37)) + 0.001 * r).astype(np.float16) for r in range(5349, 5500)])
    lo = np.stack([(base * 0.5 - r).astype(np.float16) for r in (0, 1)])
    m.bank_put(5349, hi)
    m.bank_put(0, lo)
    assert m.bank_info()["rows_filled"] == 153
    assert m.bank_get(5498, 2).tobytes() == hi[-2:].tobytes()
    rows = np.array([5499, 0, 5350, 5349, 1, 5423, 5351, 5498], np.int32)
    table = np.stack([lo[r] if r < 2 else hi[r - 5349] for r in rows])
    tb, _ = table_batch(d, len(rows), seed=191)
    tb = dict(tb, feats=table)
    mc = np.random.default_rng(1).integers(0, d["K"] + 1, (d["B"], 4)).astype(np.int32)
    got = eval_run(m, bank_of(tb, rows), mc)
    want = eval_run(m, tb, mc)
    assert not differing(got, want), differing(got, want)
    hop_w = np.full(d["H"], 1.0, np.float32)
    got = train_run(m, bank_of(tb, rows), None, hop_w, seed_step=(3, 1))
    want = train_run(m, tb, None, hop_w, seed_step=(3, 1))
    assert not differing(got, want), differing(got, want)
    m.close()


# -------------------------------------------------------------------------------------- errors
def test_bad_calls_fail_closed():
    d = SMALL
    m = make(d)
    m.evaluate()
    lib, B = m._lib, d["B"]
    tb, pb = table_batch(d, 5, seed=90)
    m.set_batch(**pb)
    m.forward()
    before = m.outputs()

    def good_step():
        """The resident batch is untouched, or (with rows) a bank batch still matches."""
        m.forward()
        assert not differing(before, m.outputs())

    args = (tb["tokens"].ctypes.data, tb["lens"].ctypes.data, tb["labels"].ctypes.data)
    idx = tb["image_of"]
    rows = np.array([3, 9, 0, 7, 5], np.int32)

    def both(n, r, i, code, what):
        r, i = np.ascontiguousarray(r, np.int32), np.ascontiguousarray(i, np.int32)
        rc = lib.rau_set_batch_bank(m._h, n, r.ctypes.data, i.ctypes.data, *args)
        assert rc == code and what.encode() in lib.rau_last_error(), (rc, lib.rau_last_error())
        assert lib.rau_set_batch_async_bank(m._h, 1, n, r.ctypes.data, i.ctypes.data, *args, 1) == code
        assert m.batch_images() == 0
        good_step()

    both(5, rows, idx, STATE, "no feature bank")                                    # no bank yet
    for fn in (lambda: lib.rau_bank_info(m._h, None, None, None), lambda: lib.rau_bank_put(m._h, 0, 1, tb["feats"].ctypes.data, 0),
               lambda: lib.rau_bank_get(m._h, 0, 1, tb["feats"].ctypes.data)):
        assert fn() == STATE
    assert lib.rau_bank_destroy(m._h) == 0                                          # nothing to do
    assert lib.rau_bank_create(m._h, 2 ** 31 - 1, 0) == NOMEM                       # 2^31 maps do not fit
    good_step()                                                                     # ... and the context is usable
    assert lib.rau_bank_create(m._h, 0, 0) == INVALID and lib.rau_bank_create(m._h, 4, 3) == INVALID
    m.bank_create(10, "f32")
    assert lib.rau_bank_create(m._h, 10, 0) == STATE                                # one bank per context
    for first, count in ((-1, 1), (10, 1), (8, 3), (0, 0)):
        assert lib.rau_bank_put(m._h, first, count, np.zeros((3, d["D"], d["S"]), np.float32).ctypes.data, 0) == INVALID
        assert lib.rau_bank_get(m._h, first, count, np.zeros((3, d["D"], d["S"]), np.float32).ctypes.data) == INVALID
    both(5, rows, idx, STATE, "never been written")
    for n, r in enumerate(rows[:4]):
        m.bank_put(int(r), tb["feats"][n:n + 1])
    both(5, rows, idx, STATE, "never been written")                                 # row 5 still is not
    m.bank_put(5, tb["feats"][4:5])
    both(5, np.where(np.arange(5) == 2, 10, rows), idx, INVALID, "bank_rows")       # a row outside the bank
    both(5, np.where(np.arange(5) == 4, -1, rows), idx, INVALID, "bank_rows")
    both(5, rows, np.where(np.arange(B) == 3, 5, idx), INVALID, "image_of")
    both(5, rows, np.where(np.arange(B) == 0, -1, idx), INVALID, "image_of")
    both(0, rows, idx, INVALID, "n_images")
    both(B + 1, np.zeros(B + 1, np.int32), idx, INVALID, "n_images")
    # the good bank batch: equal to the table batch, and its backward fails closed like the table's
    m.set_batch(**tb)
    m.forward()
    want = m.outputs()
    m.set_batch(**bank_of(tb, rows))
    m.forward()
    assert not differing(want, m.outputs())
    hop_w = np.full(d["H"], 1.0, np.float32)
    with pytest.raises(_lib.RauError, match="librau error -3.*image table"):
        m.backward(hop_w)
    m.bank_destroy()                                                                # the resident batch went with it
    with pytest.raises(_lib.RauError, match="librau error -3"):
        m.forward()
    m.set_batch(**pb)
    m.zero_grads()
    good_step()
    m.backward(hop_w)
    assert all(np.all(np.isfinite(g)) for g in m.get_grads().values())
    m.close()
