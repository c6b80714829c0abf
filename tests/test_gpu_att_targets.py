"""Attention supervision on the GPU (rau_set_att_targets, rau_backward_att, rau_graph_step_att, rau_att_stats,
rau_att_criterion_*; att_sup.hip): the attprob output trained on per-sample target maps.

The oracle is tests/att_ref.py: ref_torch's step restated in fp64 with  att_w[h] * ATT_h  added to the loss, one
run per sample with attbymemory's bias at -1e30 behind the count where the batch has region counts.
Bar: TOL = 1e-4, util.rel_err per layer slice, as tests/test_gpu_parity.py.  Condition on the inputs, asserted
for every problem (att_ref.check): in the fp64 oracle every a >= 1e-4 where t > 0; eps = 1e-12 and the float32
rounding of a then stay far below the bar.  Targets (att_ref.targets, seeded): normalised smooth rows, a one-hot
row, an un-normalised row and two all-zero rows.  hop_w = H everywhere; att_w non-uniform, no powers of two.

1. parity (every attention-backward kernel, one quad, pitched maps, a row longer than a workgroup)
2. attention loss only   3. identity with the path without it   4. the bit-for-bit statement; module level
5. region counts   6. uploads and lifetime   7. graph   8. statistics   9. bf16 mode   10. errors
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ref_torch as RT
from rau_vqa_amd import feat16, joint
from tests import att_ref, regions_ref, util
from tests.test_gpu_att_variants import SEVEN, WIDE
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_positions import F32
from tests.test_gpu_regions import BOXES

pytestmark = pytest.mark.gpu

TOL = 1e-4
STATE, INVALID = -3, -1
GROUPS = ("embed", "rnn", "mult")
ATT_ENV = ("RAU_ATT_SPLIT", "RAU_ATT_FUSED", "RAU_ATT_DMA_OFF", "RAU_ATT_CHUNKS")
BITS = ("losses", "argmax", "logits", "dopred", "att", "q", "att_c", "att_h", "g_embed", "g_rnn", "g_mult")

SHAPES = {"edge": (util.EDGE, 0.5), "small": (util.SMALL, 0.5), "seven": (SEVEN, 0.5), "wide": (WIDE, 0.3),
          "boxes": (BOXES, 0.5),
          "s195": (dict(F32, B=6, S=195), 0.2),      # a pitched 14 x 14 map: one pad column
          "s400": (dict(F32, B=6, S=400), 0.2),      # a row longer than a workgroup
          # the split family's bound, small widths: 16 trips of every row loop, targets on the last position
          "s4096": (dict(B=6, T=4, V=40, E=8, Rq=16, D=24, S=4096, M=40, A=20, R=16, K=12, H=2), 0.2)}
# Under near-uniform attention over 4096 positions no a reaches att_ref's 10 * A_MIN = 1e-3 and no target could be
# placed.  attbymemory's bias + 8 at these positions gives each of them about 1 / (10 + 4096 e^-8) = 0.09: targets()
# then places its rows on them, the last position among them, and row 0's one-hot target is moved onto it.
BOOSTED = {"s4096": (0, 255, 256, 1023, 2048, 4000, 4092, 4093, 4094, 4095)}
COUNTS = {"small": np.array([12, 7, 3, 1, 5, 12, 2, 9], np.int32),
          "boxes": np.array([100, 10, 99, 36, 1, 57, 64, 100], np.int32)}


def att_weights(H):
    return np.array([0.5, 3.0, 1.5, 0.7, 2.2, 1.1, 0.9, 1.9][:H], np.float32)


def hop_weights(H):
    return np.full(H, float(H), np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, counts=False, hop_zero=False):
    """(sh, batch, params, masks, t, n, fp64 reference) of a shape, computed once and left unchanged."""
    dims, scale = SHAPES[name]
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    if name in BOOSTED:
        from tests import range_cases
        range_cases.views(sh, params)["att_mem.b"][list(BOOSTED[name])] += 8.0
    n = COUNTS[name] if counts else None
    hop_w = np.zeros(sh.H, np.float32) if hop_zero else hop_weights(sh.H)
    fwd = att_ref.step(sh, params, batch, masks, hop_w, nreg=n, backward=False)
    t = att_ref.targets(fwd["att"], n)
    if name in BOOSTED:
        assert t[2:5, sh.S - 1].all() and set(np.flatnonzero(t.any(axis=0))) <= set(BOOSTED[name])
        t[0] = 0.0
        t[0, sh.S - 1] = 1.0
    if n is not None:                          # values behind the counts are to be ignored: make them loud
        for b, nb in enumerate(n):
            t[b, nb:] = 7.0
    assert att_ref.check(fwd["att"], t, n)
    ref = att_ref.step(sh, params, batch, masks, hop_w, att_weights(sh.H), t, nreg=n)
    return sh, batch, params, masks, t, n, ref


def make_model(dims, params, masks=None, dtype="f32", mode="train"):
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**dims, dtype=dtype))
    m.set_params(params)
    if mode == "train":
        m.training()
        if masks is not None:
            m.set_masks(masks)
    else:
        m.evaluate()
    return m


def put(m, batch, t=None, regions=None, **kw):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], regions=regions, att_targets=t, **kw)


def results(m, hop_w, att_w=None, graph=False, select_w=None):
    """zero_grads + forward + backward on the resident batch: every output and gradient."""
    if graph:
        m.graph_step(hop_w, zero_grads=True, select_w=select_w, att_w=att_w)
        out = m.outputs()
    else:
        m.zero_grads()
        m.forward()
        out = m.outputs()
        m.backward(hop_w, select_w=select_w, att_w=att_w)
    g = m.get_grads()
    out.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]})
    return out


def same_bits(a, b, keys=BITS):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def grads_differ(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ("g_embed", "g_rnn", "g_mult"))


def errors(got, ref, layouts, outputs=True):
    errs = {k: util.rel_err(got[k], ref[k]) for k in util.OUT_KEYS} if outputs else {}
    for grp in GROUPS:
        for name, sl in util.layer_slices(layouts[grp]):
            r, d = ref["g_" + grp][sl], got["g_" + grp][sl]
            errs[name] = float(np.max(np.abs(d - r))) if np.max(np.abs(r)) < 1e-12 else util.rel_err(d, r)
    return errs


def assert_within(errs, what):
    print(what, {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"{what}: relative errors above {TOL}: {bad}"


def set_env(monkeypatch, env):
    for k in ATT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)               # read when the context is created / at every launch


# ---------------------------------------------------------------- 1. parity
SPLIT_F, FUSED_F, REGS_F = "att_fwd_split", "att_fwd_fused", "att_fwd_fused_regs"
FUSED_ENV, REGS_ENV = {"RAU_ATT_FUSED": "1"}, {"RAU_ATT_FUSED": "1", "RAU_ATT_DMA_OFF": "1"}
CASES = [
    ("edge", {}, SPLIT_F),                     # S = 4: one quad, H = 1, B = 5
    ("small", {}, SPLIT_F),                    # k_att_bwd_split
    ("small", FUSED_ENV, FUSED_F),             # k_att_bwd_dma
    ("small", REGS_ENV, REGS_F),               # k_att_bwd_fused
    ("seven", {"RAU_ATT_SPLIT": "1"}, SPLIT_F),   # S = 49 at pitch 52, the three families
    ("seven", FUSED_ENV, FUSED_F),
    ("seven", REGS_ENV, REGS_F),
    ("wide", {}, FUSED_F),                     # B = 80, S = 196: fused by default
    ("s195", {}, SPLIT_F),                     # a pitched 14 x 14 map
    ("s400", {}, SPLIT_F),                     # 400 positions: the row loop of k_att_grad
    ("s4096", {}, SPLIT_F),                    # 4096 positions, targets on the last one
]


@pytest.mark.parametrize("name,env,kernel", CASES, ids=[n + "".join(" " + k[8:] for k in e) for n, e, _ in CASES])
def test_parity_with_the_reference(monkeypatch, name, env, kernel):
    set_env(monkeypatch, env)
    sh, batch, params, masks, t, _n, ref = reference(name)
    m = make_model(SHAPES[name][0], params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    put(m, batch, t)
    assert m.batch_att_targets()
    m.prof_enable()
    got = results(m, hop_weights(sh.H), att_weights(sh.H))
    m.sync()
    launched = {k: v["launches"] for k, v in m.prof().items()}
    m.close()
    bwd = "att_bwd_split" if kernel == SPLIT_F else "att_bwd_fused"
    att = {k: v for k, v in launched.items() if k.startswith("att_")}
    assert att == {kernel: sh.H, bwd: sh.H, "att_sup_grad": 1}, launched
    assert_within(errors(got, ref, layouts), name)
    ok, _, _ = util.argmax_margin_ok(ref["logits"], got["argmax"], ref["argmax"])
    assert ok
    # the term is there: the same step without it is far outside the bar
    plain = RT.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks,
                    hop_weights(sh.H)) if name == "small" else None
    assert plain is None or util.rel_err(plain["g_mult"], ref["g_mult"]) > 100 * TOL


# ---------------------------------------------------------------- 2. attention loss only
def test_attention_loss_alone():
    sh, batch, params, masks, t, _n, ref = reference("small", hop_zero=True)
    m = make_model(util.SMALL, params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    put(m, batch, t)
    got = results(m, np.zeros(sh.H, np.float32), att_weights(sh.H))
    m.close()
    assert_within(errors(got, ref, layouts, outputs=False), "hop_w = 0")
    for name, sl in util.layer_slices(layouts["mult"]):
        if name.startswith(("classifier.out_score.", "classifier.out_do_pred.")):
            assert not got["g_mult"][sl].any(), name            # exactly 0: no gradient reaches the two heads
    assert got["g_mult"].any() and got["g_rnn"].any() and got["g_embed"].any()


# ---------------------------------------------------------------- 3. identity
def test_null_and_zero_weights_are_the_path_without_them():
    sh, batch, params, masks, t, _n, _ref = reference("small")
    m = make_model(util.SMALL, params, masks)
    lib, h = m._lib, m._h
    hop_w, zeros = hop_weights(sh.H), np.zeros(sh.H, np.float32)
    hp, zp = hop_w.ctypes.data, zeros.ctypes.data

    def run(call):
        m.prof_reset()
        m.zero_grads()
        m.forward()
        out = m.outputs()
        assert call() == 0
        g = m.get_grads()
        m.sync()
        out.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]})
        return out, {k: v["launches"] for k, v in m.prof().items() if v["launches"]}
    m.prof_enable()
    put(m, batch)                                               # a batch without targets
    assert not m.batch_att_targets()
    base, listing = run(lambda: lib.rau_backward(h, hp))
    assert "att_sup_grad" not in listing
    for call in (lambda: lib.rau_backward_att(h, hp, None, None), lambda: lib.rau_backward_att(h, hp, zp, zp)):
        got, ls = run(call)
        same_bits(got, base)
        assert ls == listing
    put(m, batch, t)                                            # ... and with them
    for call in (lambda: lib.rau_backward(h, hp), lambda: lib.rau_backward_select(h, hp, None),
                 lambda: lib.rau_backward_att(h, hp, None, None), lambda: lib.rau_backward_att(h, hp, None, zp),
                 lambda: lib.rau_backward_att(h, hp, zp, zp)):
        got, ls = run(call)
        same_bits(got, base)
        assert ls == listing
    m.prof_enable(False)
    same_bits(results(m, hop_w), base)                          # the Python forms
    same_bits(results(m, hop_w, att_w=None), base)
    same_bits(results(m, hop_w, att_w=zeros), base)
    assert grads_differ(results(m, hop_w, att_w=att_weights(sh.H)), base)
    put(m, batch, np.zeros_like(t))                             # every row unsupervised: the weights change no bit
    same_bits(results(m, hop_w, att_w=att_weights(sh.H)), base)
    m.close()


# ---------------------------------------------------------------- 4. the statement, bit for bit; module level
@pytest.mark.parametrize("name", ["small", "seven"])            # dense rows of 12 (quads) and of 49 (scalar path)
def test_criterion_backward_is_the_numpy_statement_bit_for_bit(name):
    import torch
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda
    sh, batch, params, masks, t, _n, _ref = reference(name)
    n = np.random.default_rng(2).integers(1, sh.S + 1, sh.B).astype(np.int32)
    m = make_model(SHAPES[name][0], params, masks)
    put(m, batch)
    m.forward()
    a = m.attention()                                           # the device's own attention
    ext = torch.cuda.ExternalStream(m.stream(), device="cuda")
    with torch.cuda.stream(ext):
        t_dev, n_dev = cuda(t), cuda(n, torch.int32)
        for hop in range(sh.H):
            a_dev = cuda(a[hop])
            crit = modules.AttCriterionClone(m, hop)
            for counts, nd in ((None, None), (n, n_dev)):
                w = float(att_weights(sh.H)[hop])
                got = crit.backward(a_dev, t_dev, nd, w).cpu().numpy()
                want = joint.att_ce_grad(a[hop], t, w, counts)
                assert got.dtype == want.dtype == np.float32
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (hop, counts is not None)
                loss = crit.forward(a_dev, t_dev, nd)
                assert abs(loss - float(joint.att_ce(a[hop].astype(np.float64), t, counts))) < 1e-5 * abs(loss)
    m.close()


def test_step_level_equals_module_level_feval():
    import torch
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda
    sh, batch, params, masks, t, _n, ref = reference("small")
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    m = make_model(util.SMALL, params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.zero_grads()
    modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32), cuda(batch["lens"], torch.int32),
                  cuda(batch["labels"], torch.int32), hop_w, att_w=att_w, att_targets=cuda(t))
    m.sync()
    g = m.get_grads()
    g_mod = {"g_" + k: g[k] for k in GROUPS}
    put(m, batch, t)
    g_step = results(m, hop_w, att_w)
    m.close()
    assert_within(errors(g_mod, ref, layouts, outputs=False), "feval vs the oracle")
    # the two device paths against each other, on the oracle's scale per layer (attscore's bias gradient sums dz over
    # a softmax: zero in exact arithmetic, rounding noise in both, so its own norm is no scale)
    errs = {}
    for grp in GROUPS:
        for name, sl in util.layer_slices(layouts[grp]):
            den = np.max(np.abs(ref["g_" + grp][sl]))
            errs[name] = float(np.max(np.abs(g_step["g_" + grp][sl] - g_mod["g_" + grp][sl])) / (den if den >= 1e-12 else 1.0))
    assert_within(errs, "step level vs feval")


# ---------------------------------------------------------------- 5. region counts
@pytest.mark.parametrize("name", ["boxes", "small"])
def test_region_counts_against_the_per_sample_reference(name):
    sh, batch, params, masks, t, n, ref = reference(name, counts=True)
    m = make_model(SHAPES[name][0], params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    put(m, batch, t, regions=n)
    got = results(m, hop_w, att_w)
    assert_within(errors(got, ref, layouts), name + " with counts")
    # huge finite values behind the counts change no bit
    loud = t.copy()
    for b, nb in enumerate(n):
        loud[b, nb:] = 3e38
    put(m, batch, loud, regions=n)
    same_bits(results(m, hop_w, att_w), got)
    st = m.att_stats()
    put(m, batch, t, regions=n)
    m.forward()
    st2 = m.att_stats()
    m.close()
    for k in ("loss", "mass", "hits"):
        assert np.array_equal(st[k].view(np.uint32), st2[k].view(np.uint32)), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_uniform_count_is_the_bias_at_minus_1e30(dtype):
    sh, batch, params, masks, t, _n, _ref = reference("small")
    n = 7
    m = make_model(util.SMALL, params, masks, dtype=dtype)
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    put(m, batch, t, regions=np.full(sh.B, n, np.int32))
    counted = results(m, hop_w, att_w)
    cut = t.copy()
    cut[:, n:] = 0
    m.set_params(regions_ref.masked_params(sh, params, n, m.layout("mult"), dtype=np.float32))
    put(m, batch, cut)
    by_bias = results(m, hop_w, att_w)
    same_bits(counted, by_bias)
    assert grads_differ(counted, results(m, hop_w))
    m.close()


# ---------------------------------------------------------------- 6. uploads and lifetime
def test_every_upload_path_agrees_bit_for_bit():
    sh, batch, params, masks, t, _n, _ref = reference("small")
    m = make_model(util.SMALL, params, masks)
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    N = 5
    image_of = np.array([0, 1, 2, 0, 1, 3, 4, 4], np.int32)
    table = feat16.widen(feat16.fp8_bits(batch["feats"][:N], "e4m3"), "e4m3")   # values every element type holds
    feats = np.ascontiguousarray(table[image_of])
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    step = lambda: results(m, hop_w, att_w)
    m.set_batch(feats, *tok, att_targets=t)
    plain = step()
    m.set_batch(feats, *tok)
    assert grads_differ(plain, results(m, hop_w))
    m.set_batch(feats.astype(np.float16), *tok, att_targets=t)
    same_bits(plain, step())
    m.set_batch(table, *tok, image_of=image_of, att_targets=t)                  # per sample, also beside a table
    assert m.batch_images() == N and m.batch_att_targets()
    same_bits(plain, step())
    m.bank_create(N + 2)
    m.bank_put(1, table)
    m.set_batch(None, *tok, bank_rows=np.arange(1, N + 1), image_of=image_of, att_targets=t)
    same_bits(plain, step())
    m.set_batch_async(1, feats, *tok)                          # the targets go between the upload and use_batch
    m.set_att_targets(t, slot=1)
    m.use_batch(1)
    assert m.batch_att_targets()
    same_bits(plain, step())
    m.set_batch_async(0, table, *tok, image_of=image_of, att_targets=t)
    m.use_batch(0)
    same_bits(plain, step())
    m.set_batch_async(1, None, *tok, bank_rows=np.arange(1, N + 1), image_of=image_of, att_targets=t)
    m.use_batch(1)
    same_bits(plain, step())
    # set after the forward: no second forward is needed
    m.set_batch(feats, *tok)
    m.zero_grads()
    m.forward()
    out = m.outputs()
    m.set_att_targets(t)
    m.backward(hop_w, att_w=att_w)
    g = m.get_grads()
    out.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]})
    same_bits(plain, out)
    m.close()


def test_lifetime_of_the_targets_in_the_two_slots():
    sh, batch, params, masks, t, _n, _ref = reference("small")
    m = make_model(util.SMALL, params, masks)
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    args = (batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    put(m, batch, t)
    sup = results(m, hop_w, att_w)
    m.set_batch(*args)                                         # a re-upload into the slot clears them
    assert not m.batch_att_targets()
    assert m._lib.rau_graph_step_att(m._h, hop_w.ctypes.data, None, att_w.ctypes.data, 1) == STATE
    m.set_att_targets(t)
    assert m.batch_att_targets()
    same_bits(sup, results(m, hop_w, att_w))
    m.set_batch_size(sh.B - 1)                                 # ... and so does set_batch_size
    assert not m.batch_att_targets()
    m.set_batch_size(sh.B)
    m.set_masks(masks)
    m.set_batch_async(1, *args, att_targets=t)
    m.use_batch(1)
    m.set_batch_async(0, *args)                                # an upload into the other slot leaves them
    assert m.batch_att_targets()
    same_bits(sup, results(m, hop_w, att_w))
    m.use_batch(0)                                             # a batch without targets
    assert not m.batch_att_targets()
    m.use_batch(1)                                             # slot 1 still holds its own
    assert m.batch_att_targets()
    same_bits(sup, results(m, hop_w, att_w))
    m.set_batch_async(1, *args)                                # re-filled in place: gone
    assert not m.batch_att_targets()
    # a batch of n < capacity rows takes [n, S]
    k = sh.B - 3
    part = {"feats": batch["feats"][:k], "tokens": np.ascontiguousarray(batch["tokens"][:, :k]),
            "lens": batch["lens"][:k], "labels": batch["labels"][:k]}
    put(m, part, t[:k])
    assert m.batch_size == k and m.batch_att_targets()
    m.set_masks({s: np.ascontiguousarray(v[:, :k]) for s, v in masks.items()})
    small = results(m, hop_w, att_w)
    m.close()
    from rau_vqa_amd.model import RAU, Config
    m2 = RAU(Config(**dict(util.SMALL, B=k)))
    m2.set_params(params)
    m2.training()
    m2.set_masks({s: np.ascontiguousarray(v[:, :k]) for s, v in masks.items()})
    put(m2, part, t[:k])
    same_bits(small, results(m2, hop_w, att_w))
    with pytest.raises(ValueError):
        m2.set_att_targets(t)                                  # [capacity of the other context, S]: not this batch
    m2.close()


# ---------------------------------------------------------------- 7. graph
def test_graph_step_att():
    sh, batch, params, masks, t, _n, _ref = reference("small")
    m = make_model(util.SMALL, params, masks)
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    other = np.array([2.3, 0.0, 0.6], np.float32)
    put(m, batch)
    eager0 = results(m, hop_w)
    same_bits(eager0, results(m, hop_w, graph=True))            # captured WITHOUT targets first
    put(m, batch, t)
    eager = results(m, hop_w, att_w)
    eager2 = results(m, hop_w, other)
    assert grads_differ(eager, eager0) and grads_differ(eager, eager2)
    same_bits(eager0, results(m, hop_w, graph=True))            # a batch with targets, no weights: the same bits
    same_bits(eager, results(m, hop_w, att_w, graph=True))      # capture
    same_bits(eager2, results(m, hop_w, other, graph=True))     # replay with a changed att_w
    same_bits(eager, results(m, hop_w, att_w, graph=True))
    same_bits(eager0, results(m, hop_w, np.zeros(sh.H, np.float32), graph=True))
    sel = np.array([0.7, 0.0, 1.3], np.float32)                 # all three signals in one captured step
    same_bits(results(m, hop_w, att_w, select_w=sel), results(m, hop_w, att_w, graph=True, select_w=sel))
    put(m, batch)                                               # without targets again: not the supervised graph
    same_bits(eager0, results(m, hop_w, graph=True))
    assert m._lib.rau_graph_step_att(m._h, hop_w.ctypes.data, None, att_w.ctypes.data, 1) == STATE
    m.close()


# ---------------------------------------------------------------- 8. statistics
@pytest.mark.parametrize("name,counts", [("small", False), ("boxes", True), ("seven", False), ("wide", False)])
def test_att_stats_against_the_numpy_statement(name, counts):
    sh, batch, params, masks, t, n, _ref = reference(name, counts=counts)
    m = make_model(SHAPES[name][0], params, masks)
    for mode in ("train", "eval"):
        if mode == "eval":
            m.evaluate()
        put(m, batch, t, regions=n)
        m.forward()
        got = m.att_stats()
        again = m.att_stats()
        want = joint.att_stats(m.attention(), t, n)
        for k in ("loss", "mass"):
            assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k
            assert np.all(np.abs(got[k] - want[k]) <= 1e-5 * np.abs(want[k])), (mode, k, got[k], want[k])
        assert np.array_equal(got["hits"], want["hits"]) and np.array_equal(got["hits"], again["hits"]), mode
        assert got["n_sup"] == want["n_sup"] == again["n_sup"] == sh.B - 2
        assert want["loss"].min() > 0 and 0 < want["mass"].min() and want["mass"].max() <= 1 + 1e-6
    if counts:                                                  # the counts are respected: without them other numbers
        put(m, batch, t)
        m.forward()
        free = m.att_stats()
        assert not np.array_equal(free["loss"], got["loss"])
        want = joint.att_stats(m.attention(), t)
        assert np.all(np.abs(free["loss"] - want["loss"]) <= 1e-5 * np.abs(want["loss"]))
    m.close()


# ---------------------------------------------------------------- 9. bf16 mode
def test_bf16_mode_against_the_emulated_oracle():
    """The bar of tests/test_gpu_select.py's bf16 test, derived the same way from tests/test_gpu_bf16.py's
    constants: TOL_BASE + 2^-8 / sqrt(shortest reduction) + SAFETY x the largest shift of the nudged emulations."""
    sh, batch, params, masks, t, _n, _ref = reference("small")
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    m = make_model(util.SMALL, params, masks, dtype="bf16")
    layouts = {k: m.layout(k) for k in GROUPS}
    put(m, batch, t)
    got = results(m, hop_w, att_w)
    m.close()
    with RT.bf16_emulation():
        emu = att_ref.step(sh, params, batch, masks, hop_w, att_w, t, bf16=True)
    nudged = []
    for n in NUDGES:
        with RT.bf16_emulation(n):
            nudged.append(att_ref.step(sh, params, batch, masks, hop_w, att_w, t, bf16=True))
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    err = lambda a, b: float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    bad, ratio = {}, 0.0
    for grp in GROUPS:
        for name, sl in util.layer_slices(layouts[grp]):
            r = emu["g_" + grp][sl]
            flip = max(err(x["g_" + grp][sl], r) for x in nudged)
            tol = TOL_BASE + one_flip + SAFETY * flip
            e = err(got["g_" + grp][sl], r)
            ratio = max(ratio, e / tol)
            if not e < tol:
                bad[name] = (e, tol)
    print(f"bf16 attention supervision: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated oracle, (error, derived bar): {bad}"


# ---------------------------------------------------------------- 10. errors
def test_errors_leave_the_previous_targets_in_force():
    sh, batch, params, masks, t, _n, _ref = reference("small")
    m = make_model(util.SMALL, params, masks)
    lib, h = m._lib, m._h
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    hp, ap = hop_w.ctypes.data, att_w.ctypes.data
    f32 = lambda a: np.ascontiguousarray(a, np.float32)

    def rc(a, slot=-1):
        a = f32(a)
        return lib.rau_set_att_targets(h, slot, a.ctypes.data)
    out = [np.zeros(sh.H, np.float32), np.zeros(sh.H, np.float32), np.zeros(sh.H, np.int32), np.zeros(1, np.int32)]
    stats = lambda: lib.rau_att_stats(h, *[o.ctypes.data for o in out[:3]], out[3].ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc(t) == STATE and rc(t, slot=1) == STATE            # no batch in the slot
    put(m, batch)
    m.forward()
    assert stats() == STATE                                     # a forward, but no targets
    assert lib.rau_backward_att(h, hp, None, ap) == STATE       # a non-zero att_w without targets: nothing launched
    assert lib.rau_backward_att(h, hp, None, None) == 0         # ... and the forward is still there for this one
    put(m, batch, t)
    assert stats() == STATE                                     # targets, but no forward on this upload
    sup = results(m, hop_w, att_w)
    assert stats() == 0
    neg, nan, inf = t.copy(), t.copy(), t.copy()
    neg[3, 2], nan[0, 0], inf[5, 7] = -1e-6, np.nan, np.inf
    assert rc(neg) == INVALID and rc(nan) == INVALID and rc(inf) == INVALID
    assert rc(t, slot=2) == INVALID and lib.rau_set_att_targets(h, -1, None) == INVALID
    assert lib.rau_batch_att_targets(h, None) == INVALID
    assert m.batch_att_targets()
    same_bits(sup, results(m, hop_w, att_w))                    # the previous targets are still in force
    m.zero_grads()
    m.forward()
    for bad in (f32([0.5, np.nan, 1.5]), f32([np.inf, 0, 0])):
        assert lib.rau_backward_att(h, hp, None, bad.ctypes.data) == INVALID
        assert lib.rau_backward_att(h, hp, bad.ctypes.data, ap) == INVALID
        assert lib.rau_backward_att(h, bad.ctypes.data, None, ap) == INVALID
        assert lib.rau_graph_step_att(h, hp, None, bad.ctypes.data, 1) == INVALID
    assert lib.rau_backward_att(h, hp, None, ap) == 0
    assert lib.rau_backward_att(h, hp, None, ap) == STATE       # one backward per forward
    g = m.get_grads()
    for k in GROUPS:
        assert np.array_equal(g[k], sup["g_" + k]), k
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], att_targets=t)
    m.use_batch(1)
    m.forward()
    assert rc(t, slot=1) == STATE                               # current batch of a forward whose backward has not run
    assert rc(neg, slot=0) == INVALID
    assert rc(t * 2) == 0                                       # the synchronous form may follow a forward
    m.backward(hop_w, att_w=att_w)
    assert rc(t, slot=1) == 0
    with pytest.raises(ValueError):
        m.set_att_targets(t[:-1])
    m.close()
