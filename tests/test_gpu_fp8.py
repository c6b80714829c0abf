"""fp8 feature maps (RAU_FEAT_E4M3 / RAU_FEAT_E5M2, include/rau.h): a batch given as OCP e4m3fn or e5m2 codes
must give BIT-IDENTICAL results to the same batch given as f32 holding the widened values -- in every
compute mode, on both hop-copy paths of bf16 mode, with device-drawn and caller-supplied masks, on 14x14 and
pitched 7x7 maps, in training and evaluate mode, through the upload slots (4 / 2 / 1-byte batches in one
buffer), image tables, the feature bank, the captured step and the module-level calls; and rau_bank_put
narrows f32 maps to the bits of feat16.fp8_bits.  The maps are random BIT PATTERNS (every subnormal code,
+-0 and the largest finite codes included), not rounded f32 values.  Dims are those of
tests/test_gpu_feat16.py."""
import numpy as np
import pytest

import oracle
from rau_vqa_amd import feat16, synth
from tests import util
from tests.test_fp8_host import values_and_codes
from tests.test_gpu_feat16 import DIMS, KEYS, batch_of as batch_of16, make, run
from tests.test_gpu_parity import TOL
from tests.test_gpu_shared_images import differing, eval_run, index_of, train_run

pytestmark = pytest.mark.gpu

FP8 = ("e4m3", "e5m2")
INVALID = -1


def feat_bits(shape, ft, seed):
    """Random fp8 maps: mostly magnitudes in [2^-6, 4) (e4m3) / [2^-14, 4) (e5m2) of both signs, plus every
    subnormal code, +-0 and the largest finite values on fixed positions.  No NaN, no infinity."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    mbits = 3 if ft == "e4m3" else 2
    sign = rng.integers(0, 2, n).astype(np.uint8) << 7
    e = rng.integers(1, 9 if ft == "e4m3" else 17, n).astype(np.uint8)          # biased exponents: values below 4
    bits = sign | (e << mbits) | rng.integers(0, 1 << mbits, n).astype(np.uint8)
    sub = rng.integers(1, 1 << mbits, n).astype(np.uint8) | sign                 # every subnormal code turns up
    big = np.array([0x7E, 0xFE, 0x7D, 0xF8] if ft == "e4m3" else [0x7B, 0xFB, 0x7A, 0xF8], np.uint8)
    pick = rng.random(n)
    bits = np.where(pick < 0.05, sub, bits)
    bits[pick > 0.98] = np.uint8(0)
    bits[pick > 0.99] = np.uint8(0x80)
    bits[::997] = np.resize(big, bits[::997].shape)
    w = feat16.widen(bits, ft)
    assert np.all(np.isfinite(w)) and np.max(np.abs(w)) == (448.0 if ft == "e4m3" else 57344.0)
    assert set(range(1, 1 << mbits)) <= set(bits[(bits & 0x7F) < (1 << mbits)] & 0x7F)
    return bits.reshape(shape)


def batch_of(d, ft, seed):
    """(the batch as `ft`, the same batch as f32 holding the widened values)"""
    if ft not in FP8:
        return batch_of16(d, "f16" if ft == "f32" else ft, seed)
    b = synth.make_batch(d["B"], d["T"], d["V"], d["D"], d["S"], d["K"], seed=seed, lens="ragged")
    bits = feat_bits((d["B"], d["D"], d["S"]), ft, seed)
    return dict(b, feats=bits), dict(b, feats=feat16.widen(bits, ft))


def typed(d, t, seed):
    """One batch handed over as type t ("f32": the widened fp16 draw)."""
    b, b32 = batch_of(d, t, seed)
    return b32 if t == "f32" else b


def assert_same(got, want, what):
    bad = [k for k in KEYS if not np.array_equal(got[k], want[k])]
    assert not bad, f"{what}: differs in {bad}"
    for k in ("losses", "logits", "g_embed", "g_rnn", "g_mult"):
        assert np.all(np.isfinite(want[k])), k


# ---------------------------------------------------------------------------------------- 1. the step
@pytest.mark.parametrize("ft,dtype,S,masks,mode", [
    ("e4m3", "f32", 196, "device", "train"),
    ("e5m2", "f32", 49, "device", "train"),
    ("e5m2", "f32", 196, "explicit", "train"),
    ("e4m3", "f32", 49, "explicit", "train"),
    ("e4m3", "bf16", 196, "device", "train"),     # bf16 hop copies (xd16), Philox-drawing pass
    ("e5m2", "bf16", 196, "explicit", "train"),   # xd16 from caller-supplied masks
    ("e4m3", "bf16", 49, "explicit", "train"),    # bf16 mode without xd16 (pitched map)
    ("e5m2", "f32s", 196, "device", "train"),
    ("e4m3", "f32", 49, "device", "eval"),
    ("e5m2", "bf16", 196, "device", "eval"),
], ids=lambda v: str(v))
def test_step_fp8_batch_equals_widened_f32_bitwise(ft, dtype, S, masks, mode):
    d = dict(DIMS, S=S)
    m = make(d, dtype)
    if mode == "eval":
        m.evaluate()
    else:
        m.training()
        if masks == "explicit":
            sh = util.shapes(d)
            m.set_masks(synth.make_masks(oracle.mask_shapes(sh), {k: 0.5 for k in oracle.MASK_SITES}, seed=4))
    for i, seed in enumerate((1, 2)):
        b8, b32 = batch_of(d, ft, seed)
        got = run(m, b8, ft, i)
        want = run(m, b32, "f32", i)
        assert_same(got, want, f"{ft} batch {i} against the widened f32 batch")
    m.close()


# ------------------------------------------------------------------------------------------ 2. slots
def test_async_slots_switching_4_2_1_byte_batches_equal_synchronous():
    """S = 49 (pitch 52): one slot takes f32, e4m3, f16, e5m2, ... batches, in place and copied; whatever an
    earlier batch of another element size left in the buffer, pad columns included, must not show."""
    d = dict(DIMS, S=49)
    hop_w = np.full(d["H"], float(d["H"]), np.float32)
    types = ["f32", "e4m3", "f16", "e5m2", "f32", "e5m2", "e4m3", "bf16"]
    batches = [typed(d, t, 20 + i) for i, t in enumerate(types)]
    m = make(d)
    m.training()
    want = [run(m, b, t, i, hop_w) for i, (b, t) in enumerate(zip(batches, types))]

    def fill(slot, i):
        b, t = batches[i], types[i]
        if i % 2:                                          # in place, in the slot's typed staging
            v = m.batch_slot(slot, feat_type=t)
            assert v["feats"].dtype == feat16.dtype_of(t) and v["feats"].shape == (d["B"], d["D"], d["S"])
            for k in ("feats", "tokens", "lens", "labels"):
                v[k][...] = np.asarray(b[k]).reshape(v[k].shape)
            m.set_batch_async(slot, feat_type=t)
        else:
            m.set_batch_async(slot, **b, feat_type=t)

    def step(i):
        assert m.batch_feat_type() == types[i]
        m.set_dropout_seed(31, i)
        m.zero_grads()
        m.forward()
        out = m.outputs()
        m.backward(hop_w)
        return {**out, **{"g_" + k: v for k, v in m.get_grads().items()}}
    for i in range(len(batches)):                          # every batch through slot 0
        fill(0, i)
        m.use_batch(0)
        assert_same(step(i), want[i], f"slot 0, step {i} ({types[i]})")
    fill(1, 0)
    for i in range(len(batches)):                          # alternating slots, the next upload under the step
        m.use_batch((i + 1) & 1)
        if i + 1 < len(batches):
            fill(i & 1, i + 1)
        assert_same(step(i), want[i], f"alternating slots, step {i} ({types[i]})")
    m.close()


# ------------------------------------------------------------------------------------ 3. image tables
def table_batch(d, N, ft, seed):
    b = synth.make_batch(d["B"], d["T"], d["V"], d["D"], d["S"], d["K"], seed=seed, lens="ragged")
    table = feat_bits((N, d["D"], d["S"]), ft, seed + 1)
    image_of = index_of(d["B"], N, seed + 2)
    return dict(b, feats=table, image_of=image_of, feat_type=ft), dict(b, feats=table[image_of], feat_type=ft)


def mc_of(d, seed):
    return np.random.default_rng(seed).integers(0, d["K"] + 1, (d["B"], 4)).astype(np.int32)


@pytest.mark.parametrize("ft,S", [("e4m3", 49), ("e5m2", 196)])
def test_image_table_equals_plain_batch(ft, S):
    d = dict(DIMS, S=S)
    hop_w = np.array([3.0, 1.0, 3.0], np.float32)
    m = make(d)
    tb, pb = table_batch(d, 5, ft, seed=50)
    got, want = eval_run(m, tb, mc_of(d, 1)), eval_run(m, pb, mc_of(d, 1))      # per-image convolution
    assert not differing(got, want), f"evaluate: table differs from feats[image_of] in {differing(got, want)}"
    got = train_run(m, tb, None, hop_w, seed_step=(13, 2))                        # expansion on the device
    assert m.batch_images() == 5 and m.batch_feat_type() == ft
    want = train_run(m, pb, None, hop_w, seed_step=(13, 2))
    assert not differing(got, want), f"train: table differs from feats[image_of] in {differing(got, want)}"
    assert all(np.all(np.isfinite(got[k])) and np.any(got[k] != 0) for k in ("g_embed", "g_rnn", "g_mult"))
    m.close()


# --------------------------------------------------------------------------------------------- 4. bank
@pytest.mark.parametrize("S", [196, 49])
def test_bank_put_get_and_device_narrowing(S):
    d = dict(DIMS, S=S)
    per = d["D"] * S
    m = make(d)
    rng = np.random.default_rng(S)
    for ft in FP8:
        codes = rng.integers(0, 256, (6, d["D"], S)).astype(np.uint8)               # any code, NaNs included: a copy
        m.bank_create(8, ft)
        assert m.bank_info() == {"capacity": 8, "feat_type": ft, "rows_filled": 0}
        m.bank_put(4, codes[4:6], feat_type=ft)
        m.bank_put(0, codes[0:4], feat_type=ft)
        got = m.bank_get(0, 6)
        assert got.dtype == np.uint8 and got.tobytes() == codes.tobytes(), ft
        assert not m.bank_get(6, 2).any()                                           # never written: zeros
        m.bank_destroy()
        # f32 in: narrowed on the device to feat16.fp8_bits, bit for bit
        x, want_cases = values_and_codes(ft)
        bits = rng.integers(0, 2 ** 32, 5 * per, dtype=np.uint64).astype(np.uint32)  # every exponent, inf and NaN too
        vals = bits.view(np.float32).copy()
        vals[::3] = (rng.standard_normal(vals[::3].size) * 10.0 ** rng.uniform(-6, 5, vals[::3].size)).astype(np.float32)
        assert x.size < per
        vals[:x.size] = x                                                            # the cases of the host test
        src = vals.reshape(5, d["D"], S)
        want = feat16.fp8_bits(src, ft)
        m.bank_create(5, ft)
        m.bank_put(0, src)
        got = m.bank_get(0, 5)
        nan = np.isnan(src)
        assert nan.any() and np.isinf(src).any()
        bad = np.flatnonzero((got != want).ravel() & ~nan.ravel())
        assert bad.size == 0, (ft, bad.size, [(float(vals[i]), hex(got.ravel()[i]), hex(want.ravel()[i])) for i in bad[:8]])
        assert np.all(np.isnan(feat16.widen(got[nan], ft)))
        np.testing.assert_array_equal(got.ravel()[:x.size][~np.isnan(x)], want_cases[~np.isnan(x)])
        assert np.all(np.isfinite(feat16.widen(got[~nan], ft)))                      # saturating: no infinity comes out
        m.bank_destroy()
    m.close()


@pytest.mark.parametrize("ft,S,put_f32", [("e4m3", 196, False), ("e5m2", 49, False), ("e4m3", 49, True)])
def test_bank_batch_equals_table_batch_equals_plain_batch(ft, S, put_f32):
    d = dict(DIMS, S=S)
    hop_w = np.array([3.0, 1.0, 3.0], np.float32)
    m = make(d)
    tb, pb = table_batch(d, 5, ft, seed=70)
    rows = np.array([7, 2, 11, 0, 5], np.int32)
    m.bank_create(12, ft)
    for n in np.random.default_rng(3).permutation(5):
        if put_f32:   # the widened maps plus less than half an ulp: the device narrows them back to the same codes
            w = feat16.widen(tb["feats"][n:n + 1], ft)
            m.bank_put(int(rows[n]), (w * np.float32(1 + 2.0 ** -6)).astype(np.float32))
        else:
            m.bank_put(int(rows[n]), tb["feats"][n:n + 1], feat_type=ft)
    assert m.bank_get(int(rows[3]), 1).tobytes() == tb["feats"][3:4].tobytes()
    bank = {k: v for k, v in tb.items() if k not in ("feats", "feat_type")}
    bank = dict(bank, feats=None, bank_rows=rows)
    got = eval_run(m, bank, mc_of(d, 2))
    assert m.batch_images() == 5 and m.batch_feat_type() == ft
    table, plain = eval_run(m, tb, mc_of(d, 2)), eval_run(m, pb, mc_of(d, 2))
    assert not differing(got, table), f"evaluate: bank batch differs from the table batch in {differing(got, table)}"
    assert not differing(got, plain), f"evaluate: bank batch differs from the plain batch in {differing(got, plain)}"
    got = train_run(m, bank, None, hop_w, seed_step=(5, 1))
    table = train_run(m, tb, None, hop_w, seed_step=(5, 1))
    plain = train_run(m, pb, None, hop_w, seed_step=(5, 1))
    assert not differing(got, table), f"train: bank batch differs from the table batch in {differing(got, table)}"
    assert not differing(got, plain), f"train: bank batch differs from the plain batch in {differing(got, plain)}"
    assert all(np.all(np.isfinite(got[k])) for k in got)
    m.close()


def test_fp8_bank_survives_set_batch_size():
    d = dict(DIMS, S=49)
    m = make(d)
    tb, _ = table_batch(d, 5, "e4m3", seed=80)
    m.bank_create(6, "e4m3")
    m.bank_put(1, tb["feats"], feat_type="e4m3")                  # filled BEFORE the resize
    m.set_batch_size(8)
    assert m.bank_info() == {"capacity": 6, "feat_type": "e4m3", "rows_filled": 5}
    assert m.bank_get(1, 5).tobytes() == tb["feats"].tobytes()
    d8 = dict(d, B=8)
    tb8, pb8 = table_batch(d8, 5, "e4m3", seed=80)                # the same table, 8 questions
    assert tb8["feats"].tobytes() == tb["feats"].tobytes()
    bank = {k: v for k, v in tb8.items() if k not in ("feats", "feat_type")}
    got = eval_run(m, dict(bank, feats=None, bank_rows=(np.arange(5) + 1).astype(np.int32)), mc_of(d8, 3))
    want = eval_run(m, pb8, mc_of(d8, 3))
    assert not differing(got, want), differing(got, want)
    m.close()


# ------------------------------------------------------------------------------------ 5. captured step
def test_graph_step_with_fp8_batches_matches_eager():
    """The key of a captured step holds the element type: after a captured f16 step an e4m3 batch of the
    same shape is captured anew and gives the e4m3 eager bits, not a replay of the f16 graph."""
    d = DIMS
    hop_w = np.full(d["H"], 2.0, np.float32)
    eager, graph = make(d), make(d)
    for m in (eager, graph):
        m.training()
    lens = np.full(d["B"], d["T"], np.int32)     # one longest-question length: one graph per type
    seq = [(dict(typed(d, t, 60 + i), lens=lens), t) for i, t in enumerate(["f16", "e4m3", "e5m2", "f16", "e4m3", "f32"])]
    for it, (b, t) in enumerate(seq):
        outs = []
        for m, use_graph in ((eager, False), (graph, True)):
            m.set_batch(**b, feat_type=t)
            m.set_dropout_seed(11, it)
            if use_graph:
                m.graph_step(hop_w)
            else:
                m.zero_grads()
                m.forward()
                m.backward(hop_w)
            g = m.get_grads()
            outs.append((m.losses(), m.logits(), g["embed"], g["rnn"], g["mult"]))
        for a, b_ in zip(*outs):
            assert np.all(np.isfinite(a)) and np.array_equal(a, b_), f"step {it} ({t})"
    eager.close()
    graph.close()


# ------------------------------------------------------------------------------------- 6. module level
@pytest.mark.parametrize("ft,S", [("e4m3", 49), ("e5m2", 196)])
def test_module_level_calls_on_the_resident_fp8_batch(ft, S):
    """rau_multimodal_forward / _backward with X = NULL read the resident batch."""
    import torch
    from rau_vqa_amd import modules
    d = dict(DIMS, S=S, H=2)
    m = make(d)
    m.training()
    m.set_dropout_seed(8, 1)
    rng = np.random.default_rng(2)
    c = m.cfg
    q = torch.as_tensor(rng.uniform(-1, 1, (c.B, c.Q)).astype(np.float32)).cuda()
    dl = torch.as_tensor(rng.uniform(-1, 1, (c.B, c.K)).astype(np.float32)).cuda()
    da = torch.as_tensor(rng.uniform(-1, 1, (c.B, c.S)).astype(np.float32)).cuda()
    b8, b32 = batch_of(d, ft, 6)

    def clone_run(batch, t):
        m.set_batch(**batch, feat_type=t)
        m.zero_grads()
        outs = []
        for h in range(c.H):
            mm = modules.MultimodalClone(m, h)
            fwd = mm.forward(q, None, None, None)             # logits, do_pred, attprob, c', h'
            m.sync()                                           # (the ctx stream, not torch's)
            outs += [x.cpu().numpy().copy() for x in fwd]
            bwd = mm.backward(q, None, None, None, dl, d_attprob=da, want_dX=True)   # dq, dX, dc, dh
            m.sync()
            outs += [x.cpu().numpy().copy() for x in bwd]
        g = m.get_grads()
        return outs + [g["mult"]]

    got, want = clone_run(b8, ft), clone_run(b32, "f32")
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a, b)]
    assert not bad, f"module-level outputs {bad} differ"
    assert all(np.all(np.isfinite(a)) for a in want)
    m.close()


# ------------------------------------------------------------------------------------------ 7. oracle
def test_fp8_batch_against_the_oracle():
    """The whole path, not only self-consistency: an e4m3 batch against the fp64 oracle on the widened
    input, at the f32 parity bar."""
    sh = util.shapes(util.MEDIUM)
    batch, params, masks = util.make_problem(sh, scale=0.2)
    bits = feat16.fp8_bits(batch["feats"], "e4m3")      # the dataset stored as e4m3
    wide = feat16.widen(bits, "e4m3")
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    ref = oracle.step(sh, params, wide, batch["tokens"], batch["lens"], batch["labels"], masks, hop_w,
                      dtype=np.float64)
    m = make(util.MEDIUM, params=params)
    m.training()
    m.set_masks(masks)
    m.set_batch(bits, batch["tokens"], batch["lens"], batch["labels"], feat_type="e4m3")
    assert m.batch_feat_type() == "e4m3"
    m.zero_grads()
    m.forward()
    m.backward(hop_w)
    out, g = m.outputs(), m.get_grads()
    errs = {"losses": util.rel_err(out["losses"], ref["losses"]),
            "logits": util.rel_err(out["logits"], ref["logits"]),
            **{"g_" + k: util.rel_err(g[k], ref["g_" + k]) for k in g}}
    print("e4m3 batch vs fp64 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"fp8 batch vs oracle above {TOL}: {bad}"
    ok, _, _ = util.argmax_margin_ok(ref["logits"], out["argmax"], ref["argmax"])
    assert ok
    m.close()


# -------------------------------------------------------------------------------------- 8. rejections
def test_unknown_types_and_conversions_the_bank_does_not_make_are_rejected():
    d = dict(DIMS, B=4, H=1)
    m = make(d)
    b = synth.make_batch(d["B"], d["T"], d["V"], d["D"], d["S"], d["K"], seed=9, lens="ragged")
    lib = m._lib
    f = b["feats"]
    tok, lens, lab = (np.ascontiguousarray(b[k], np.int32) for k in ("tokens", "lens", "labels"))
    for ft in (3, 6):                                           # 3 is reserved, 6 is beyond the enum
        rc = lib.rau_set_batch_typed(m._h, f.ctypes.data, ft, tok.ctypes.data, lens.ctypes.data, lab.ctypes.data)
        assert rc == INVALID and b"feat_type" in lib.rau_last_error() and b"_E4M3" in lib.rau_last_error()
        rc = lib.rau_set_batch_async_typed(m._h, 0, f.ctypes.data, ft, tok.ctypes.data, lens.ctypes.data,
                                           lab.ctypes.data, 1)
        assert rc == INVALID and b"feat_type" in lib.rau_last_error()
        assert lib.rau_bank_create(m._h, 4, ft) == INVALID
    one = np.clip(f[:1], -100, 100)
    codes = feat16.fp8_bits(one, "e4m3")
    for bank_ft, src, src_ft in (("e4m3", one.astype(np.float16), 1), ("e5m2", codes, 4), ("e4m3", codes, 5),
                                 ("e5m2", feat16.bf16_bits(one), 2), ("f32", codes, 4), ("f16", codes, 5)):
        m.bank_create(2, bank_ft)
        assert lib.rau_bank_put(m._h, 0, 1, src.ctypes.data, src_ft) == INVALID, (bank_ft, src_ft)
        assert m.bank_info()["rows_filled"] == 0
        m.bank_destroy()
    with pytest.raises(ValueError, match="e4m3"):
        m.set_batch(codes.repeat(d["B"], 0), b["tokens"], b["lens"], b["labels"])        # uint8 without a name
    with pytest.raises(ValueError):
        m.bank_put(0, codes)
    m.set_batch(codes.repeat(d["B"], 0), b["tokens"], b["lens"], b["labels"], feat_type="e4m3")
    assert m.batch_feat_type() == "e4m3"
    m.close()
