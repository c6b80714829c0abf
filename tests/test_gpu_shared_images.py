"""Batches that share feature maps between the questions of one image (rau_set_batch_images /
rau_set_batch_async_images, include/rau.h): a batch given as an image table feats [N,D,S] + image_of [B]
must give BIT-IDENTICAL results to the plain batch feats[image_of] -- on the evaluate-mode fast path
(convolutions once per image, attention tiles read through the device index), in train mode and through
the captured step (table gathered on the device), through the upload slots and the module-level calls --
and bad tables are rejected before anything is uploaded.  Every case draws one seeded input and runs it
both ways; the expansion is done here with numpy."""
import ctypes as C

import numpy as np
import pytest

import oracle
from rau_vqa_amd import _lib, feat16, synth
from tests import util
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

# the model's channel width and map at small recurrent widths (M, A, R off the tile sizes)
D512 = dict(B=48, T=9, V=300, E=200, Rq=64, D=512, S=196, M=136, A=132, R=68, K=1000, H=3)
REAL = dict(T=26, V=14000, E=200, Rq=512, D=512, S=196, M=512, A=256, R=512, K=1000, H=8)   # configs[0]
SMALL = dict(B=12, T=9, V=300, E=200, Rq=64, D=72, S=196, M=136, A=132, R=68, K=1000, H=3)
EVAL_KEYS = ("losses", "logits", "argmax", "dopred", "att", "q", "att_c", "att_h")


def make(dims, dtype="f32", seed=5):
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**dims, dtype=dtype))
    m.init_uniform(seed=seed, lo=-0.05, hi=0.05)
    return m


def index_of(B, N, seed, kind="shuffle"):
    """image_of [B]: every table row is looked at, repeats are not adjacent."""
    rng = np.random.default_rng(seed)
    if kind == "perm":
        assert N == B
        return rng.permutation(B).astype(np.int32)
    idx = np.concatenate([np.arange(N), rng.integers(0, N, B - N)])
    return rng.permutation(idx).astype(np.int32)


def table_batch(d, N, seed, ft="f32", kind="shuffle"):
    """(table batch, plain batch) of one seeded draw: the same tokens / lens / labels, feats [N,D,S] with
    image_of against feats[image_of]."""
    b = synth.make_batch(d["B"], d["T"], d["V"], d["D"], d["S"], d["K"], seed=seed, lens="ragged")
    table = synth.make_batch(N, 1, 2, d["D"], d["S"], 2, seed=seed + 1)["feats"]
    if ft == "f16":
        table = table.astype(np.float16)
    elif ft == "bf16":
        table = feat16.bf16_bits(table)
    image_of = index_of(d["B"], N, seed + 2, kind)
    kw = {} if ft == "f32" else {"feat_type": ft}
    return dict(b, feats=table, image_of=image_of, **kw), dict(b, feats=table[image_of], **kw)


def eval_run(m, batch, mc, prof=False):
    m.evaluate()
    m.set_batch(**batch)
    if prof:
        m.prof_enable(True)
        m.prof_reset()
    m.forward()
    out = m.outputs()
    if prof:
        out["_prof"] = m.prof()
        m.prof_enable(False)
    st = m.step_stats()
    out.update({"st_" + k: np.asarray(v) for k, v in st.items()})
    out["oe"], out["mc"] = m.predict(mc)
    out["m_pred"], out["m_att"] = m.merged()
    return out


def differing(a, b):
    return [k for k in a if not k.startswith("_") and not np.array_equal(a[k], b[k])]


def eval_case(d, N, seed, ft="f32", dtype="f32", kind="shuffle", kernel=None):
    m = make(d, dtype)
    tb, pb = table_batch(d, N, seed, ft, kind)
    mc = np.random.default_rng(seed).integers(0, d["K"] + 1, (d["B"], 4)).astype(np.int32)
    got = eval_run(m, tb, mc, prof=kernel is not None)       # first, in a fresh context: rows >= N of I / P are unwritten
    assert m.batch_images() == N
    want = eval_run(m, pb, mc)
    assert m.batch_images() == 0
    if kernel:                                               # the attention kernel family that served the table run
        other = "att_fwd_split" if kernel == "att_fwd_fused" else "att_fwd_fused"
        assert got["_prof"][kernel]["launches"] == d["H"] and other not in got["_prof"]
        convs = got["_prof"]["conv_embed_fwd"]
        assert convs["launches"] == 1                        # once per image, not per sample or hop:
        assert convs["flops"] == 2.0 * d["M"] * N * d["S"] * d["D"]
    bad = differing(got, want)
    assert not bad, f"table batch differs from feats[image_of] in {bad}"
    m.close()
    return got, pb


# ------------------------------------------------------------------------------- evaluate mode
def test_eval_b48_n16_split_kernels_and_the_oracle():
    """B = 48 (the split attention kernels), N = 16, D = 512, 14 x 14: bitwise against the plain batch, and
    the expanded batch against the fp64 oracle at the project's bar."""
    d = D512
    m = make(d)
    params = m.get_params()
    m.close()
    got, pb = eval_case(d, 16, seed=40, kernel="att_fwd_split")
    sh = util.shapes(d)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    ref = oracle.step(sh, params, pb["feats"], pb["tokens"], pb["lens"], pb["labels"], None, hop_w,
                      dtype=np.float64)
    errs = {k: util.rel_err(got[k], ref[k]) for k in util.OUT_KEYS}
    print("table batch vs fp64 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), errs
    assert np.array_equal(got["argmax"], ref["argmax"])


def test_eval_7x7_maps_pitched_rows():
    eval_case(dict(D512, S=49), 16, seed=41)


def test_eval_d2048_bf16_mode():
    eval_case(dict(D512, D=2048, M=256, A=64), 16, seed=42, dtype="bf16")


def test_eval_b144_n48_real_widths_fused_kernels():
    """configs[0] widths at B = 144 (above 64 samples: the fused LDS-DMA attention kernels), N = 48."""
    eval_case(dict(REAL, B=144), 48, seed=43, kernel="att_fwd_fused")


def test_eval_permutation_n_equals_b():
    eval_case(D512, 48, seed=44, kind="perm")


def test_eval_one_image_for_the_whole_batch():
    eval_case(D512, 1, seed=45)


@pytest.mark.parametrize("ft,S", [("f16", 196), ("bf16", 49)])
def test_eval_16bit_tables(ft, S):
    eval_case(dict(SMALL, B=80, S=S), 27, seed=46, ft=ft)


# ---------------------------------------------------------------------------------- train mode
def train_run(m, batch, masks, hop_w, graph=False, seed_step=None):
    m.training()
    if masks is not None:
        m.set_masks(masks)
    if seed_step is not None:
        m.set_dropout_seed(*seed_step)
    m.set_batch(**batch)
    if graph:
        m.graph_step(hop_w)
    else:
        m.zero_grads()
        m.forward()
        m.backward(hop_w)
    g = m.get_grads()
    return {"losses": m.losses(), "logits": m.logits(), "att": m.attention(), "g_embed": g["embed"],
            "g_rnn": g["rnn"], "g_mult": g["mult"]}


@pytest.mark.parametrize("S,ft", [(196, "f32"), (49, "f16")])
def test_train_forward_backward_explicit_masks(S, ft):
    d = dict(SMALL, S=S)
    sh = util.shapes(d)
    _, _, masks = util.make_problem(sh, seed=9)
    hop_w = np.array([3.0, 1.0, 3.0], np.float32)
    m = make(d)
    tb, pb = table_batch(d, 5, seed=50, ft=ft)
    got = train_run(m, tb, masks, hop_w)
    want = train_run(m, pb, masks, hop_w)
    bad = differing(got, want)
    assert not bad, f"train step on a table batch differs in {bad}"
    m.close()


def test_graph_step_replays_with_a_new_index_and_a_new_n():
    d = SMALL
    hop_w = np.full(d["H"], 3.0, np.float32)
    mg, me = make(d), make(d)
    lens = np.full(d["B"], d["T"], np.int32)               # one longest length: one graph shape
    graphs = None
    for it, N in enumerate((5, 5, 9)):                      # new index, then a new N: both replay
        tb, pb = table_batch(d, N, seed=60 + it)
        tb["lens"] = pb["lens"] = lens
        got = train_run(mg, tb, None, hop_w, graph=True, seed_step=(13, it))
        want = train_run(me, pb, None, hop_w, seed_step=(13, it))
        bad = differing(got, want)
        assert not bad, f"replay {it}: captured step on a table batch differs in {bad}"
    mg.close()
    me.close()


# --------------------------------------------------------------------------------------- slots
def test_slots_table_and_plain_alternate():
    d = dict(SMALL, B=20)
    ma, ms = make(d), make(d)
    ma.evaluate()
    ms.evaluate()
    for it in range(4):
        slot = it & 1
        tb, pb = table_batch(d, 7, seed=70 + it, ft="f16" if it == 2 else "f32")
        batch = dict(tb if slot == 0 else pb)               # slot 0 holds tables, slot 1 plain batches
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
        want = ms.outputs()
        bad = differing(got, want)
        assert not bad, f"step {it} (slot {slot}) differs from the synchronous plain batch in {bad}"
    ma.close()
    ms.close()


# -------------------------------------------------------------------------------- module level
def test_multimodal_forward_on_the_resident_table_batch():
    import torch
    from rau_vqa_amd import modules
    d = dict(SMALL, H=2)
    m = make(d)
    m.training()
    m.set_dropout_seed(8, 1)
    c = m.cfg
    q = torch.as_tensor(np.random.default_rng(2).uniform(-1, 1, (c.B, c.Q)).astype(np.float32)).cuda()
    tb, pb = table_batch(d, 4, seed=80)

    def clone_run(batch):
        m.set_batch(**batch)
        outs = []
        for h in range(c.H):
            fwd = modules.MultimodalClone(m, h).forward(q, None, None, None)   # X = NULL: the resident batch
            m.sync()
            outs += [x.cpu().numpy().copy() for x in fwd]
        return outs
    got, want = clone_run(tb), clone_run(pb)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a, b)]
    assert not bad, f"module-level outputs {bad} differ"
    m.close()


# -------------------------------------------------------------------------------------- errors
def test_bad_tables_are_rejected_and_backward_fails_closed():
    d = SMALL
    m = make(d)
    m.evaluate()
    tb, pb = table_batch(d, 5, seed=90)
    m.set_batch(**pb)
    m.forward()
    before = m.outputs()
    lib, B = m._lib, d["B"]
    args = (tb["tokens"].ctypes.data, tb["lens"].ctypes.data, tb["labels"].ctypes.data)
    big = np.zeros((B + 1, d["D"], d["S"]), np.float32)
    for n, idx, what in ((5, np.where(np.arange(B) == 3, 5, tb["image_of"]), "image_of"),
                         (5, np.where(np.arange(B) == 0, -1, tb["image_of"]), "image_of"),
                         (0, np.zeros(B, np.int32), "n_images"),
                         (B + 1, np.zeros(B, np.int32), "n_images")):
        idx = np.ascontiguousarray(idx, np.int32)
        rc = lib.rau_set_batch_images(m._h, big.ctypes.data, 0, n, idx.ctypes.data, *args)
        assert rc == -1 and what.encode() in lib.rau_last_error(), (n, lib.rau_last_error())   # RAU_ERR_INVALID
        rc = lib.rau_set_batch_async_images(m._h, 1, big.ctypes.data, 0, n, idx.ctypes.data, *args, 1)
        assert rc == -1
    assert m.batch_images() == 0
    m.forward()                                              # the resident batch is untouched
    assert not differing(before, m.outputs())
    # fail closed: no per-sample I behind the fast path
    m.set_batch(**tb)
    m.forward()
    hop_w = np.full(d["H"], 1.0, np.float32)
    with pytest.raises(_lib.RauError, match="librau error -3.*image table"):
        m.backward(hop_w)
    # a plain batch afterwards works, gradients included
    m.set_batch(**pb)
    m.zero_grads()
    m.forward()
    assert not differing(before, m.outputs())
    m.backward(hop_w)
    assert all(np.all(np.isfinite(g)) for g in m.get_grads().values())
    m.close()
