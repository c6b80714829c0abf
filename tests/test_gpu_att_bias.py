"""The caller's attention bias on the GPU (rau_set_att_bias_dev): bias[b, s] joins sample b's attention score at
position s in every hop, -inf masks the position, and every backward leaves the gradient at the bias.

1. parity      against tests/bias_ref.py (one run of the unchanged fp64 oracle per sample, the bias added to
               attbymemory's bias, -inf as -1e30): tests/test_gpu_parity.py's 1e-4 max-norm relative bar on every
               output, every layer's gradient and d_bias, train and evaluate mode, in each forward attention kernel;
2. counts      bias and region counts together; NaN behind the counts changes no bit;
3. identities  bit for bit: a +0 bias is no bias; -inf behind n[b] is set_regions(n); rows are independent; two
               backwards give the same d_bias; a batch without a bias launches what the parent commit did;
4. bf16 mode   at the bar tests/test_gpu_state.py derives for that mode;
5. lifetime and refusals;  6. captured steps;  7. together with the other per-batch attachments;  8. autograd;
9. module level.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from tests import bias_ref, state_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_regions import (BITS, FUSED, PARENT_LAUNCHES, REGS, SHAPES, SPLIT, assert_same_bits, differs,
                                    hop_weights, make, results, set_mode)

pytestmark = pytest.mark.gpu

TOL = 1e-4
STATE, INVALID = -3, -1
ENV_KNOBS = ("RAU_ATT_SPLIT", "RAU_ATT_FUSED", "RAU_ATT_DMA_OFF", "RAU_ATT_CHUNKS")


# ------------------------------------------------------------------------------------------ machinery
def bias_of(name):
    """bias_ref.pattern at the shape: one finite position (row 0), alternate -inf (1), a mask edge that is no multiple
    of 4 (2), the last logical position only (3: in front of seven's pad columns), zeros (4), 2 * normal elsewhere."""
    dims = SHAPES[name][0]
    return bias_ref.pattern(dims["B"], dims["S"])


def counts_of(name):
    """Region counts that leave every row of bias_of(name) a finite entry: S on rows 0 and 3, ragged elsewhere."""
    return {"small": np.array([12, 7, 3, 12, 5, 12, 2, 9], np.int32),
            "boxes": np.array([100, 10, 99, 100, 1, 57, 64, 100], np.int32)}[name]


def dev(a, dtype=torch.float32):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()
    torch.cuda.synchronize()            # the upload ran on torch's stream: done before the ctx reads it
    return t


def load(m, batch, mode, masks, bias=None, regions=None, **kw):
    """The batch, then (it detaches one) the bias: numpy goes through the checked upload, a tensor is attached as is."""
    set_mode(m, mode, masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], regions=regions, **kw)
    if bias is not None:
        m.set_att_bias(bias, regions=regions if isinstance(bias, np.ndarray) else None)
        assert m.batch_att_bias


def step(m, hop_w, graph=False, backward=True):
    out = results(m, hop_w, graph, backward)
    if m.batch_att_bias and (graph or backward):
        out["d_bias"] = m.att_bias_grad()
    return out


def run(m, batch, mode, masks, hop_w, bias=None, regions=None, graph=False, **kw):
    load(m, batch, mode, masks, bias, regions, **kw)
    return step(m, hop_w, graph)


def assert_masked(att, bias, n=None):
    """Attention exactly +0 where the bias is -inf (and behind the counts), positive elsewhere."""
    off = np.isneginf(bias)
    if n is not None:
        off = off | (np.arange(bias.shape[1])[None, :] >= np.asarray(n)[:, None])
    assert np.all(att[:, off] == 0) and not np.signbit(att[:, off]).any()
    assert np.all(att[:, ~off] > 0)


def grad_layer_errs(got, ref, layouts):
    errs = {}
    for grp in ("embed", "rnn", "mult"):
        for lname, sl in util.layer_slices(layouts[grp]):
            r, d = ref["g_" + grp][sl], got["g_" + grp][sl]
            errs[lname] = float(np.max(np.abs(d - r))) if np.max(np.abs(r)) < 1e-12 else util.rel_err(d, r)
    return errs


def assert_parity(got, ref, layouts, keys=util.OUT_KEYS):
    errs = {k: util.rel_err(got[k], ref[k]) for k in keys}
    errs.update(grad_layer_errs(got, ref, layouts))
    assert np.max(np.abs(ref["d_bias"])) > 0
    errs["d_bias"] = util.rel_err(got["d_bias"], ref["d_bias"])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"


# ------------------------------------------------------------------------------------------ 1. parity
@functools.lru_cache(maxsize=None)
def reference(name, mode, with_counts=False):
    dims, scale = SHAPES[name]
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    n = counts_of(name) if with_counts else None
    return bias_ref.step(sh, params, batch, masks if mode == "train" else None, hop_weights(sh), bias_of(name), n)


F1, OFF = {"RAU_ATT_FUSED": "1"}, {"RAU_ATT_FUSED": "1", "RAU_ATT_DMA_OFF": "1"}
CASES = [
    ("small", {}, SPLIT, "train"), ("small", {}, SPLIT, "eval"),
    ("small", F1, FUSED, "train"), ("small", F1, FUSED, "eval"),
    ("small", OFF, REGS, "train"), ("small", OFF, REGS, "eval"),
    ("seven", {}, SPLIT, "train"), ("seven", {}, SPLIT, "eval"),
    ("seven", F1, FUSED, "train"), ("seven", F1, FUSED, "eval"),
    ("seven", OFF, REGS, "train"), ("seven", OFF, REGS, "eval"),
    ("wide", {}, FUSED, "train"), ("wide", {}, FUSED, "eval"),                # B = 80: the fused family by default
    ("wide", {"RAU_ATT_SPLIT": "1"}, SPLIT, "train"), ("wide", {"RAU_ATT_SPLIT": "1"}, SPLIT, "eval"),
    ("boxes", {}, SPLIT, "train"), ("boxes", {}, SPLIT, "eval"),              # S = 100
    ("boxes900", F1, REGS, "train"), ("boxes900", F1, REGS, "eval"),          # register-staged, four trips
    ("boxes4096", {}, SPLIT, "train"),                                        # split, sixteen trips
]


def set_env(monkeypatch, env):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)               # read when the context is created / at every launch


@pytest.mark.parametrize("name,env,kernel,mode", CASES,
                         ids=[n + "".join(" " + k[8:] for k in e) + " " + md for n, e, _, md in CASES])
def test_parity_with_the_per_sample_reference(monkeypatch, name, env, kernel, mode):
    set_env(monkeypatch, env)
    dims, scale = SHAPES[name]
    bias = bias_of(name)
    ref = reference(name, mode)
    m, sh, batch, params, masks = make(dims, scale=scale)
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    m.prof_enable()
    got = run(m, batch, mode, masks, hop_weights(sh), bias=bias)
    m.sync()
    launched = {k: v["launches"] for k, v in m.prof().items() if k.startswith("att_fwd")}
    tail = m.prof().get("att_bias_grad", {}).get("launches")
    m.close()
    assert launched == {kernel: sh.H}, launched
    assert tail == 1
    assert_masked(got["att"], bias)
    assert np.all(got["att"][:, 0, 2] == np.float32(1.0))      # row 0: one finite position
    assert np.all(got["d_bias"][np.isneginf(bias)] == 0)
    assert_parity(got, ref, layouts)
    ok, _, _ = util.argmax_margin_ok(ref["logits"], got["argmax"], ref["argmax"])
    assert ok, "argmax mismatch on a decided row"


# ------------------------------------------------------------------------------------------ 2. with region counts
@pytest.mark.parametrize("name", ["small", "boxes"])
def test_bias_and_counts_together_and_nan_behind_the_counts(name):
    dims, scale = SHAPES[name]
    bias, n = bias_of(name), counts_of(name)
    m, sh, batch, params, masks = make(dims, scale=scale)
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    hop_w = hop_weights(sh)
    got = run(m, batch, "train", masks, hop_w, bias=bias, regions=n)
    assert_masked(got["att"], bias, n)
    assert_parity(got, reference(name, "train", True), layouts)
    junk = bias.copy()
    for b, nb in enumerate(n):
        junk[b, nb:] = np.nan
    assert np.isnan(junk).any()
    keep = dev(junk)                                           # the device form: values nobody can check
    again = run(m, batch, "train", masks, hop_w, bias=keep, regions=n)
    m.close()
    assert_same_bits(got, again, BITS + ("d_bias",))


# ------------------------------------------------------------------------------------------ 3. identities
@pytest.mark.parametrize("name", ["small", "wide"])
def test_zero_bias_is_no_bias_and_no_bias_launches_what_the_parent_did(name):
    dims, scale = SHAPES[name]
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    m.prof_enable()
    plain = run(m, batch, "train", masks, hop_w)
    m.sync()
    listing = {k: v["launches"] for k, v in m.prof().items()}
    m.prof_enable(False)
    assert not m.batch_att_bias
    zero = run(m, batch, "train", masks, hop_w, bias=np.zeros((sh.B, sh.S), np.float32))
    assert_same_bits(plain, zero)
    assert zero["d_bias"].shape == (sh.B, sh.S) and np.abs(zero["d_bias"]).max() > 0
    assert_same_bits(run(m, batch, "eval", masks, hop_w),
                     run(m, batch, "eval", masks, hop_w, bias=dev(np.zeros((sh.B, sh.S)), torch.bfloat16)))
    m.close()
    print(listing)
    assert listing == PARENT_LAUNCHES[name]


@pytest.mark.parametrize("name,dtype,mode", [("small", "f32", "train"), ("small", "bf16", "train"),
                                             ("seven", "f32", "eval"), ("seven", "bf16", "train")])
def test_minus_inf_behind_a_count_is_set_regions(name, dtype, mode):
    dims, scale = SHAPES[name]
    m, sh, batch, params, masks = make(dims, dtype=dtype, scale=scale)
    hop_w = hop_weights(sh)
    n = np.array([sh.S, 7, 3, 1, 5, sh.S - 1, 2, 9], np.int32)[:sh.B]
    bias = np.where(np.arange(sh.S)[None, :] < n[:, None], np.float32(0), np.float32(-np.inf))
    counted = run(m, batch, mode, masks, hop_w, regions=n)
    by_bias = run(m, batch, mode, masks, hop_w, bias=bias)
    load(m, batch, mode, masks)
    m.set_att_mask(np.isfinite(bias))
    by_mask = step(m, hop_w)
    m.close()
    assert_same_bits(counted, by_bias)
    assert_same_bits(counted, by_mask)
    assert np.array_equal(by_bias["d_bias"], by_mask["d_bias"])


def test_rows_are_independent_and_two_backwards_give_the_same_bits():
    dims, scale = SHAPES["small"]
    bias = bias_of("small")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    a = run(m, batch, "train", masks, hop_w, bias=bias)
    a2 = step(m, hop_w)                                        # the bias survives a second forward
    assert_same_bits(a, a2, BITS + ("d_bias",))
    other = bias.copy()
    other[3] = bias[5]                                         # only sample 3's bias changes
    b = run(m, batch, "train", masks, hop_w, bias=other)
    m.close()
    rows = [r for r in range(sh.B) if r != 3]
    for k in ("logits", "att", "att_c", "att_h"):
        assert np.array_equal(a[k][:, rows], b[k][:, rows]), k
        assert not np.array_equal(a[k][:, 3], b[k][:, 3]), k
    assert np.array_equal(a["d_bias"][rows], b["d_bias"][rows])


# ------------------------------------------------------------------------------------------ 4. bf16 mode
@pytest.mark.parametrize("name", ["small", "wide"])
def test_bf16_mode_against_the_emulated_reference(name):
    """bf16 mode: d_bias, att, logits and every layer slice of the three gradient groups, each at its own derived bar
    (tests/test_gpu_state.py's procedure: TOL_BASE + one flip + SAFETY x the largest shift of the nudged emulations)."""
    dims, scale = SHAPES[name]
    bias = bias_of(name)
    m, sh, batch, params, masks = make(dims, dtype="bf16", scale=scale)
    hop_w = hop_weights(sh)
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    out = run(m, batch, "train", masks, hop_w, bias=bias)
    m.close()

    def tensors(res):
        t = {k: np.asarray(res[k]) for k in ("d_bias", "att", "logits")}
        for grp in layouts:
            for lname, sl in util.layer_slices(layouts[grp]):
                t[lname] = np.asarray(res["g_" + grp][sl])
        return t

    got = tensors(out)
    with RT.bf16_emulation():
        emu = tensors(bias_ref.torch_step(sh, params, batch, masks, hop_w, bias, bf16=True))
    nudged = []
    for nudge in NUDGES:
        with RT.bf16_emulation(nudge):
            nudged.append(tensors(bias_ref.torch_step(sh, params, batch, masks, hop_w, bias, bf16=True)))
    err = lambda a, b: float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    bad, ratio = {}, 0.0
    for k in got:
        flip = max(err(t[k], emu[k]) for t in nudged)
        tol = TOL_BASE + one_flip + SAFETY * flip
        e = err(got[k], emu[k])
        ratio = max(ratio, e / tol)
        print(f"bf16 {k}: error {e:.2e}, derived bar {tol:.2e} (nudged shift {flip:.2e})")
        if not e < tol:
            bad[k] = (e, tol)
    print(f"bf16: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated reference, (error, derived bar): {bad}"
    assert_masked(out["att"], bias)


# ------------------------------------------------------------------------------------------ 5. lifetime, refusals
def grad_rc(m):
    p, pitch = C.c_void_p(), C.c_int32()
    return m._lib.rau_att_bias_grad_dev(m._h, C.byref(p), C.byref(pitch)), p.value, pitch.value


def test_lifetime_of_the_bias_and_of_its_gradient():
    dims, scale = SHAPES["seven"]                              # pitched: 49 positions in rows of 52
    bias = bias_of("seven")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    args = (batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    free = run(m, batch, "train", masks, hop_w)
    assert grad_rc(m)[0] == STATE                              # a backward, but without a bias
    with pytest.raises(L.RauError):
        m.att_bias_grad()
    biased = run(m, batch, "train", masks, hop_w, bias=bias)
    assert differs(free, biased)
    rc, p, pitch = grad_rc(m)
    assert rc == 0 and p and pitch == 52
    view = m.att_bias_grad_tensor()
    assert tuple(view.shape) == (sh.B, sh.S) and view.stride(0) == 52
    m.sync()
    assert np.array_equal(view.cpu().numpy(), biased["d_bias"])
    m.forward()
    assert grad_rc(m)[0] == STATE                              # no backward since the last forward
    m.backward(hop_w)
    assert np.array_equal(m.att_bias_grad(), biased["d_bias"])
    m.set_att_bias(np.flip(bias, 0).copy())                    # attaching again replaces the contents
    assert grad_rc(m)[0] == STATE                              # ... and what a backward left is another bias's
    flipped = step(m, hop_w)
    assert differs(flipped, biased)
    m.clear_att_bias()
    assert not m.batch_att_bias
    assert_same_bits(free, step(m, hop_w))
    m.set_att_bias(bias)
    m.set_batch(*args)                                         # a re-upload detaches it
    assert not m.batch_att_bias
    assert_same_bits(free, step(m, hop_w))
    m.set_att_bias(bias)
    m.set_batch_async(1, *args)
    assert m.batch_att_bias                                    # an upload into the other slot leaves it
    m.use_batch(1)                                             # ... making that batch current does not
    assert not m.batch_att_bias
    m.use_batch(0)
    assert not m.batch_att_bias
    assert_same_bits(free, step(m, hop_w))
    m.set_att_bias(bias)
    m.set_batch_size(sh.B - 1)                                 # and so does a changed batch size
    assert not m.batch_att_bias
    m.set_batch_size(sh.B)
    assert_same_bits(biased, run(m, batch, "train", masks, hop_w, bias=bias), BITS + ("d_bias",))
    m.close()


def test_refusals_change_nothing():
    dims, scale = SHAPES["small"]
    bias = bias_of("small")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    lib, f32t, e4m3 = m._lib, 0, 3
    t = dev(np.concatenate([bias.ravel(), np.zeros(4, np.float32)]))
    assert lib.rau_set_att_bias_dev(m._h, t.data_ptr(), f32t) == STATE         # no resident batch
    biased = run(m, batch, "train", masks, hop_w, bias=bias)
    assert lib.rau_set_att_bias_dev(None, t.data_ptr(), f32t) == INVALID
    assert lib.rau_set_att_bias_dev(m._h, t.data_ptr(), e4m3) == INVALID       # fp8
    assert lib.rau_set_att_bias_dev(m._h, t.data_ptr(), 4) == INVALID
    assert lib.rau_set_att_bias_dev(m._h, t.data_ptr(), 99) == INVALID
    assert lib.rau_set_att_bias_dev(m._h, t.data_ptr() + 4, f32t) == INVALID   # not 16-byte aligned
    assert lib.rau_batch_att_bias(m._h, None) == INVALID
    assert lib.rau_get_att_bias_grad(m._h, None) == INVALID
    assert m.batch_att_bias
    assert np.array_equal(m.att_bias_grad(), biased["d_bias"])                 # the gradient is still there
    assert_same_bits(biased, step(m, hop_w), BITS + ("d_bias",))               # and so is the bias
    for bad in (bias[:-1], torch.zeros(sh.B, sh.S), dev(bias)[:, :-1], dev(bias, torch.float64)):
        with pytest.raises(ValueError):
            m.set_att_bias(bad)
    m.set_regions(np.full(sh.B, sh.S, np.int32))
    with pytest.raises(ValueError, match="regions="):
        m.set_att_bias(bias)                                   # numpy input on a batch with counts: they are needed
    m.close()


# ------------------------------------------------------------------------------------------ 6. captured steps
def test_graph_step_with_a_bias_and_its_key_member():
    """A twin context runs every step eagerly (tests/test_gpu_step_key.py's walk, for this one member): captured
    without a bias, then with one, a replay with another bias, and back."""
    dims, scale = SHAPES["small"]
    bias = bias_of("small")
    other = np.flip(bias, 0).copy()
    eager, sh, batch, params, masks = make(dims, scale=scale)
    graph = make(dims, scale=scale)[0]
    hop_w = hop_weights(sh)
    seen = []
    for b in [None, bias, other, None, bias, None]:
        outs = []
        for m in (eager, graph):
            load(m, batch, "train", masks, b)
            outs.append(step(m, hop_w, graph=m is graph))
        keys = BITS + (("d_bias",) if b is not None else ())
        assert_same_bits(outs[0], outs[1], keys)
        if b is not None:
            seen.append(outs[1]["d_bias"])
    assert not np.array_equal(seen[0], seen[1])                # the replay read the new bias
    # re-attaching between replays, the batch untouched: no recapture is needed, the new contents are read
    for m in (eager, graph):
        load(m, batch, "train", masks, bias)
    first = step(graph, hop_w, graph=True)
    graph.set_att_bias(other)
    eager.set_att_bias(other)
    assert differs(first, step(graph, hop_w, graph=True))
    assert_same_bits(step(eager, hop_w), step(graph, hop_w, graph=True), BITS + ("d_bias",))
    eager.close()
    graph.close()


# ------------------------------------------------------------------------------------------ 7. together with
def small_problem():
    dims, scale = SHAPES["small"]
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    return dims, scale, sh, batch, params, masks, bias_of("small")


def assert_close(got, ref, what, tol=TOL):
    e = util.rel_err(got, ref)
    print(f"{what}: rel_err {e:.2e}")
    assert np.max(np.abs(ref)) > 0 and e < tol, (what, e)


def test_together_with_an_attached_question_and_state():
    dims, scale, sh, batch, params, masks, bias = small_problem()
    rng = np.random.default_rng(4)
    q = (0.5 * rng.standard_normal((sh.B, 4 * sh.Rq))).astype(np.float32)
    c0 = (0.5 * rng.standard_normal((sh.B, sh.R))).astype(np.float32)
    h0 = np.tanh(rng.standard_normal((sh.B, sh.R))).astype(np.float32)
    hop_w = hop_weights(sh)
    ref = bias_ref.torch_step(sh, params, batch, masks, hop_w, bias, q=q, c0=c0, h0=h0)
    m = make(dims, scale=scale)[0]
    layouts = {"mult": m.layout("mult")}
    load(m, batch, "train", masks, bias)
    keep = (dev(q), dev(c0), dev(h0))
    m.set_question(keep[0])
    m.set_state(keep[1], keep[2])
    assert m.batch_att_bias and m.batch_question and m.batch_state
    got = step(m, hop_w)
    gq, (gc, gh) = m.question_grad(), m.state_grad()
    m.close()
    for k in ("logits", "att", "att_c", "att_h", "d_bias"):
        assert_close(got[k], ref[k], k)
    assert_close(gq, ref["g_q"], "dq")
    assert_close(gc, ref["d_c0"], "d_c0")
    assert_close(gh, ref["d_h0"], "d_h0")
    for lname, sl in util.layer_slices(layouts["mult"]):     # (attscore's bias has no gradient: a softmax's shift)
        r, d = ref["g_mult"][sl], got["g_mult"][sl]
        e = float(np.max(np.abs(d - r))) if np.max(np.abs(r)) < 1e-12 else util.rel_err(d, r)
        assert e < TOL, (lname, e)


def test_together_with_tied_dropout():
    dims, scale, sh, batch, params, masks, bias = small_problem()
    hop_w = hop_weights(sh)
    one = dict(masks, x=np.ascontiguousarray(masks["x"][0]))
    every = dict(masks, x=np.ascontiguousarray(np.broadcast_to(one["x"], (sh.H,) + one["x"].shape)))
    ref = bias_ref.step(sh, params, batch, every, hop_w, bias)
    m = make(dims, scale=scale)[0]
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    m.tie_feature_dropout()
    got = run(m, batch, "train", one, hop_w, bias=bias)
    m.close()
    assert_parity(got, ref, layouts, keys=("losses", "logits", "dopred", "att", "att_c", "att_h"))


def test_together_with_attention_targets_and_an_external_attprob_gradient():
    from tests import att_ref
    dims, scale, sh, batch, params, masks, bias = small_problem()
    hop_w, att_w = hop_weights(sh), [0.5, 3.0, 1.5]
    fwd = bias_ref.step(sh, params, batch, masks, hop_w, bias)
    t = att_ref.targets(fwd["att"])                            # targets only where the biased attention is not small
    assert att_ref.check(fwd["att"], t)
    G = (np.random.default_rng(5).normal(size=(sh.H, sh.B, sh.S)) / sh.B).astype(np.float32)
    ref = bias_ref.torch_step(sh, params, batch, masks, hop_w, bias, att_w=att_w, att_t=t,
                              F=state_ref.linear_F(G_a=G))
    m = make(dims, scale=scale)[0]
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    load(m, batch, "train", masks, bias, att_targets=t)
    assert m.batch_att_bias
    m.zero_grads()
    m.forward()
    keep = dev(G)
    m.backward(hop_w, att_w=np.asarray(att_w, np.float32), out_grads={"attprob": keep})
    got = m.outputs()
    g = m.get_grads()
    got.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"], "d_bias": m.att_bias_grad()})
    m.close()
    assert_parity(got, ref, layouts, keys=("logits", "dopred", "att", "att_c", "att_h"))


def test_together_with_an_image_table_in_evaluate_mode():
    """The conv runs per image, the bias stays per sample: two questions about one image get their own rows."""
    dims, scale, sh, batch, params, masks, bias = small_problem()
    hop_w = hop_weights(sh)
    image_of = np.array([0, 1, 2, 0, 1, 3, 4, 4], np.int32)
    table = np.ascontiguousarray(batch["feats"][:5])
    per_sample = dict(batch, feats=np.ascontiguousarray(table[image_of]))
    m = make(dims, scale=scale)[0]
    plain = run(m, per_sample, "eval", masks, hop_w, bias=bias)
    load(m, dict(batch, feats=table), "eval", masks, None, image_of=image_of)
    assert m.batch_images() == 5
    m.set_att_bias(bias)
    tab = results(m, hop_w, backward=False)
    m.close()
    for k in ("logits", "att", "att_c", "att_h", "argmax"):
        assert np.array_equal(plain[k], tab[k]), k
    assert not np.array_equal(tab["att"][:, 6], tab["att"][:, 7])   # one image, two bias rows
    assert_masked(tab["att"], bias)


# ------------------------------------------------------------------------------------------ 8. autograd
def test_autograd_step_trains_a_prior_in_front_of_the_bias():
    from rau_vqa_amd import autograd
    dims, scale, sh, batch, params, masks, _ = small_problem()
    hop_w = hop_weights(sh)
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)).cuda()
    geometry = torch.rand(sh.B, sh.S, 4, device="cuda")        # a box per position
    m = make(dims, scale=scale)[0]
    m.want_feature_grad()
    set_mode(m, "train", masks)
    x = dev(batch["feats"]).requires_grad_(True)
    b = net(geometry).squeeze(-1).contiguous()                 # [n, S], a non-leaf that requires grad
    b.retain_grad()
    own = torch.cuda.ExternalStream(m.stream())
    own.wait_stream(torch.cuda.current_stream())               # the ctx reads what torch's stream wrote
    m.set_batch_dev(x.detach(), batch["tokens"], batch["lens"], batch["labels"], att_bias=b.detach())
    m.zero_grads()
    logits, dopred, attprob = autograd.step(m, hop_w, att_bias=b, feats=x)
    (0.0 * logits.sum()).backward()                            # the built-in criterion alone, through one backward()
    torch.cuda.synchronize()
    m.sync()
    d_bias = m.att_bias_grad()
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    g = m.get_grads()
    m.close()
    assert b.grad is not None and x.grad is not None           # both arrive in the one loss.backward()
    assert np.array_equal(b.grad.cpu().numpy(), d_bias)
    assert all(p.grad is not None and p.grad.abs().max() > 0 for p in net.parameters())
    value = b.detach().cpu().numpy()
    ref = bias_ref.torch_step(sh, params, batch, masks, hop_w, value, want_feats=True)
    assert_close(d_bias, ref["d_bias"], "b.grad")
    assert_close(x.grad.cpu().numpy(), ref["g_feats"], "x.grad")
    errs = grad_layer_errs({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]}, ref, layouts)
    assert all(v < TOL for v in errs.values()), errs


# ------------------------------------------------------------------------------------------ 9. module level
def test_multimodal_clone_takes_a_bias():
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda, make_model
    name = "seven"                                             # pitched: the bias is re-pitched on its way in
    dims, scale = SHAPES[name]
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    bias = bias_of(name)
    n = np.array([49, 48, 30, 49, 5, 17], np.int32)
    ref, ref_n = reference(name, "train"), bias_ref.step(sh, params, batch, masks, hop_weights(sh), bias, n)
    m = make_model(sh, params, masks)
    feats = cuda(batch["feats"])
    ext = torch.cuda.ExternalStream(m.stream(), device=feats.device)
    with torch.cuda.stream(ext):
        q = cuda(ref["q"].astype(np.float32))
        mm = modules.MultimodalClone(m, 0)
        b_dev, n_dev = cuda(bias), cuda(n, torch.int32)
        lg, _, att, _, _ = mm.forward(q, feats, None, None, bias=b_dev)
        got = {"logits": lg.cpu().numpy(), "att": att.cpu().numpy()}
        lg, _, att, _, _ = mm.forward(q, feats, None, None, regions=n_dev, bias=b_dev)
        got_n = {"logits": lg.cpu().numpy(), "att": att.cpu().numpy()}
        lg, _, att, _, _ = mm.forward(q, feats, None, None, regions=n_dev)
        by_regions = (lg.cpu().numpy(), att.cpu().numpy())
        outs = [C.c_void_p() for _ in range(5)]
        p = lambda t: None if t is None else t.data_ptr()
        L.check(m._lib.rau_multimodal_forward_bias(m._h, 0, p(q), p(feats), None, None, p(n_dev), None,
                                                   *[C.byref(o) for o in outs]))
        null_bias = (mm._view(outs[0], sh.B, sh.K).cpu().numpy(), mm._view(outs[2], sh.B, sh.S).cpu().numpy())
        assert m._lib.rau_multimodal_forward_bias(m._h, 0, p(q), p(feats), None, None, None, p(b_dev) + 4,
                                                  *[C.byref(o) for o in outs]) == INVALID
    m.sync()
    m.close()
    for k in ("logits", "att"):
        assert_close(got[k], ref[k][0], "hop 0 " + k)
        assert_close(got_n[k], ref_n[k][0], "hop 0 with counts " + k)
    assert_masked(got["att"][None], bias)
    assert_masked(got_n["att"][None], bias, n)
    assert np.array_equal(null_bias[0], by_regions[0]) and np.array_equal(null_bias[1], by_regions[1])
