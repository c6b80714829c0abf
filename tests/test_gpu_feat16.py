"""16-bit feature maps (rau_set_batch_typed / rau_set_batch_async_typed, include/rau.h): a batch given
as fp16 or bf16 must give BIT-IDENTICAL results to the same batch given as f32 holding the widened
values -- in every compute mode, on both hop-copy paths of bf16 mode, with device-drawn and
caller-supplied masks, on 14x14 and pitched 7x7 maps, in training and evaluate mode, through the
module-level calls, the asynchronous slots and the captured step.  The maps are random BIT PATTERNS
(fp16 subnormals, +-0 and values near +-65504 included), not rounded f32 values."""
import ctypes as C

import numpy as np
import pytest

import oracle
from rau_vqa_amd import feat16, synth
from tests import util
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

# M = 136 with S = 196: RAU_BF16 stores the hop copies as bf16 (xd16); S = 49 (row pitch 52) does not
DIMS = dict(B=12, T=9, V=300, E=200, Rq=64, D=72, S=196, M=136, A=132, R=68, K=1000, H=3)
KEYS = ("losses", "logits", "argmax", "dopred", "att", "q", "att_c", "att_h", "g_embed", "g_rnn", "g_mult")


def feat_bits(shape, ft, seed):
    """Random 16-bit maps: mostly magnitudes in [2^-14, 4) (fp16) / [2^-20, 4) (bf16) of both signs,
    plus subnormals, +-0 and the largest finite values on fixed positions."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    sign = rng.integers(0, 2, n).astype(np.uint16) << 15
    if ft == "f16":
        e = rng.integers(1, 17, n).astype(np.uint16)                 # biased exponents 1..16
        bits = sign | (e << 10) | rng.integers(0, 1 << 10, n).astype(np.uint16)
        sub = rng.integers(1, 1 << 10, n).astype(np.uint16) | sign    # subnormals
        big = np.array([0x7BFF, 0xFBFF, 0x7BFE, 0xFBF0], np.uint16)   # +-65504 and neighbours
    else:
        e = rng.integers(107, 129, n).astype(np.uint16)
        bits = sign | (e << 7) | rng.integers(0, 1 << 7, n).astype(np.uint16)
        sub = rng.integers(1, 1 << 7, n).astype(np.uint16) | sign
        big = np.array([0x4780, 0xC77F, 0x46FF, 0xC6A0], np.uint16)   # +-65536 and below
    pick = rng.random(n)
    bits = np.where(pick < 0.05, sub, bits)
    bits[pick > 0.98] = np.uint16(0)
    bits[pick > 0.99] = np.uint16(0x8000)
    bits[::997] = np.resize(big, bits[::997].shape)
    bits = bits.reshape(shape)
    return bits.view(np.float16) if ft == "f16" else bits


def make(dims, dtype="f32", params=None):
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**dims, dtype=dtype))
    if params is None:
        m.init_uniform(seed=5, lo=-0.05, hi=0.05)
    else:
        m.set_params(params)
    return m


def batch_of(d, ft, seed):
    b = synth.make_batch(d["B"], d["T"], d["V"], d["D"], d["S"], d["K"], seed=seed, lens="ragged")
    bits = feat_bits((d["B"], d["D"], d["S"]), ft, seed)
    return dict(b, feats=bits), dict(b, feats=feat16.widen(bits, ft))


def run(m, batch, ft, it=0, hop_w=None):
    m.set_batch(**batch, feat_type=ft)
    assert m.batch_feat_type() == ft
    m.set_dropout_seed(31, it)
    m.zero_grads()
    m.forward()
    out = m.outputs()
    m.backward(np.full(m.cfg.H, 2.0, np.float32) if hop_w is None else hop_w)
    return {**out, **{"g_" + k: v for k, v in m.get_grads().items()}}


def assert_same(got, want, what):
    bad = [k for k in KEYS if not np.array_equal(got[k], want[k])]
    assert not bad, f"{what}: 16-bit batch differs from the widened f32 batch in {bad}"
    for k in ("losses", "g_mult"):
        assert np.all(np.isfinite(want[k])), k


@pytest.mark.parametrize("ft,dtype,S,masks,mode", [
    ("f16", "f32", 196, "device", "train"),
    ("bf16", "f32", 49, "device", "train"),
    ("bf16", "f32", 196, "explicit", "train"),
    ("f16", "bf16", 196, "device", "train"),      # bf16 hop copies (xd16), Philox-drawing pass
    ("bf16", "bf16", 196, "explicit", "train"),   # xd16 from caller-supplied masks
    ("f16", "bf16", 49, "explicit", "train"),     # bf16 mode without xd16 (pitched map)
    ("bf16", "f32s", 196, "device", "train"),
    ("f16", "f32", 49, "device", "eval"),
    ("bf16", "bf16", 196, "device", "eval"),
], ids=lambda v: str(v))
def test_step_16bit_batch_equals_widened_f32_bitwise(ft, dtype, S, masks, mode):
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
        b16, b32 = batch_of(d, ft, seed)
        got = run(m, b16, ft, i)
        want = run(m, b32, "f32", i)
        assert_same(got, want, f"batch {i}")
    m.close()


@pytest.mark.parametrize("ft,S", [("f16", 49), ("bf16", 196)])
def test_module_level_calls_on_the_resident_16bit_batch(ft, S):
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
    b16, b32 = batch_of(d, ft, 6)

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

    got, want = clone_run(b16, ft), clone_run(b32, "f32")
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a, b)]
    assert not bad, f"module-level outputs {bad} differ"
    m.close()


def test_async_slots_alternating_f32_and_f16_equal_synchronous():
    d = DIMS
    hop_w = np.full(d["H"], float(d["H"]), np.float32)
    types = ["f32", "f16", "f32", "f16", "bf16", "f16"]
    batches = []
    for i, t in enumerate(types):
        b16, b32 = batch_of(d, "f16" if t == "f32" else t, 20 + i)
        batches.append(b32 if t == "f32" else b16)
    m = make(d)
    m.training()
    want = [run(m, b, t, i, hop_w) for i, (b, t) in enumerate(zip(batches, types))]

    def fill(slot, i):
        b, t = batches[i], types[i]
        if i % 2:                                          # in place, in the slot's typed staging
            v = m.batch_slot(slot, feat_type=t)
            for k in ("feats", "tokens", "lens", "labels"):
                v[k][...] = np.asarray(b[k]).reshape(v[k].shape)
            m.set_batch_async(slot, feat_type=t)
        else:
            m.set_batch_async(slot, **b, feat_type=t)
    fill(0, 0)
    for i in range(len(batches)):
        m.use_batch(i & 1)
        assert m.batch_feat_type() == types[i]
        if i + 1 < len(batches):
            fill((i + 1) & 1, i + 1)
        m.set_dropout_seed(31, i)
        m.zero_grads()
        m.forward()
        out = m.outputs()
        m.backward(hop_w)
        got = {**out, **{"g_" + k: v for k, v in m.get_grads().items()}}
        assert_same(got, want[i], f"async step {i} ({types[i]})")
    m.close()


@pytest.mark.parametrize("S", [196, 49])
def test_pitched_pad_columns_survive_type_switches(S):
    """The 16-bit map occupies the first half of the f32 buffer: switching types in one buffer must
    leave nothing in the next batch's pad columns (S = 49: pitch 52), in either direction."""
    d = dict(DIMS, S=S, H=2)
    m = make(d)
    m.evaluate()
    b16, b32 = batch_of(d, "f16", 3)
    other16, other32 = batch_of(d, "f16", 4)
    want = run(m, b32, "f32")
    m.set_batch(**other16, feat_type="f16")
    assert_same(run(m, b32, "f32"), want, "f32 after f16")
    want16 = run(m, b16, "f16")
    m.set_batch(**other32)
    assert_same(run(m, b16, "f16"), want16, "f16 after f32")
    m.close()


def test_graph_step_with_16bit_batches_matches_eager():
    """The captured step reads the batch in its element type: its key holds the type, so switching
    the resident type captures again instead of replaying the other type's graph."""
    d = DIMS
    hop_w = np.full(d["H"], 2.0, np.float32)
    eager, graph = make(d), make(d)
    for m in (eager, graph):
        m.training()
    lens = np.full(d["B"], d["T"], np.int32)     # one longest-question length: one graph per type
    seq = []
    for i, t in enumerate(["f16", "f32", "bf16", "f16", "f32"]):
        b16, b32 = batch_of(d, "f16" if t == "f32" else t, 60 + i)
        seq.append((dict(b32 if t == "f32" else b16, lens=lens), t))
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
            assert np.array_equal(a, b_), f"step {it} ({t})"
    eager.close()
    graph.close()


def test_16bit_batch_against_the_oracle():
    """The whole path, not only self-consistency: an fp16 batch against the fp64 oracle on the widened
    input, at the f32 parity bar."""
    sh = util.shapes(util.MEDIUM)
    batch, params, masks = util.make_problem(sh, scale=0.2)
    bits = batch["feats"].astype(np.float16)          # the dataset stored as fp16
    wide = feat16.widen(bits, "f16")
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    ref = oracle.step(sh, params, wide, batch["tokens"], batch["lens"], batch["labels"], masks, hop_w,
                      dtype=np.float64)
    m = make(util.MEDIUM, params=params)
    m.training()
    m.set_masks(masks)
    m.set_batch(bits, batch["tokens"], batch["lens"], batch["labels"])   # float16 -> "f16"
    assert m.batch_feat_type() == "f16"
    m.zero_grads()
    m.forward()
    m.backward(hop_w)
    out, g = m.outputs(), m.get_grads()
    errs = {"losses": util.rel_err(out["losses"], ref["losses"]),
            "logits": util.rel_err(out["logits"], ref["logits"]),
            **{"g_" + k: util.rel_err(g[k], ref["g_" + k]) for k in g}}
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"16-bit batch vs oracle above {TOL}: {bad}"
    ok, _, _ = util.argmax_margin_ok(ref["logits"], out["argmax"], ref["argmax"])
    assert ok
    m.close()


def test_typed_entry_points_reject_unknown_types():
    d = dict(DIMS, B=4, H=1)
    m = make(d)
    b = synth.make_batch(d["B"], d["T"], d["V"], d["D"], d["S"], d["K"], seed=9, lens="ragged")
    lib = m._lib
    f = b["feats"]
    tok, lens, lab = (np.ascontiguousarray(b[k], np.int32) for k in ("tokens", "lens", "labels"))
    for ft in (3, -1):
        rc = lib.rau_set_batch_typed(m._h, f.ctypes.data, ft, tok.ctypes.data, lens.ctypes.data,
                                     lab.ctypes.data)
        assert rc == -1 and b"feat_type" in lib.rau_last_error()
        rc = lib.rau_set_batch_async_typed(m._h, 0, f.ctypes.data, ft, tok.ctypes.data, lens.ctypes.data,
                                           lab.ctypes.data, 1)
        assert rc == -1 and b"feat_type" in lib.rau_last_error()
    v = C.c_int(-5)
    assert lib.rau_batch_feat_type(m._h, C.byref(v)) == 0 and v.value == 0
    with pytest.raises(ValueError, match="bf16"):
        m.set_batch(f.view(np.uint16)[..., ::2].copy(), b["tokens"], b["lens"], b["labels"])
    m.close()
