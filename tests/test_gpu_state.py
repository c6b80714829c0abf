"""The open hop recurrence on the GPU: rau_set_state_dev (state_attach), rau_state_dev, rau_backward_state,
rau_state_grad_dev / rau_get_state_grad (state_grad_finish), autograd.step(state=, return_state=True).

Reference: tests/state_ref.py, ext_ref's fp64 autograd restatement with (c0, h0) as leaves and the hop states among
F's arguments.  Whole tensors are compared with util.rel_err at TOL = 1e-4 (g_mult per layer slice), in bf16 mode at
the derived bar of tests/test_gpu_bf16.py (TOL_BASE + ONE_FLIP + SAFETY x the largest shift of the nudged
emulations), as tests/test_gpu_question.py uses it.

Shapes: util.SMALL (M != R, H = 3), SMALL with M = 16 (M == R: hop 0 takes the batched dg launch), util.EDGE (H = 1:
hop 0 is also the last hop), test_gpu_featgrad's X196 (the 14x14 kernels) and SMALL with B = 66 (the other side of
the 64-sample switch).  The attached states are the fp64 oracle's own final (c, h) of ANOTHER random batch, so they
have the scale of real states.  Masks are explicit unless a case says otherwise.  Every group that attaches a state
has cases whose state arrives as float16 or bfloat16 (the reference then starts from the widened values), among them
util.EDGE, where n R / 4 = 5 is odd and state_attach's last quad takes the 8-byte load.

One refusal of the header is not asserted: rau_set_state_dev while a step is being captured.  The capture window opens
and closes inside one rau_graph_step* call, the context is not shared between threads, and no callback runs inside the
window, so no call of a test can land in it; the check is the one line in front of rau_set_question_dev's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from tests import question_ref, state_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_featgrad import X196
from tests.test_gpu_select import INVALID, STATE, TOL, f32, grad_errs, make_model, same_bits

pytestmark = pytest.mark.gpu

SHAPES = {"SMALL": (util.SMALL, 0.5), "M16": (dict(util.SMALL, M=16), 0.5), "EDGE": (util.EDGE, 0.5),
          "X196": (X196, 0.3), "B66": (dict(util.SMALL, B=66), 0.5), "H2": (dict(util.SMALL, H=2), 0.5),
          "H4": (dict(util.SMALL, H=4), 0.5)}
HOP_W = [3, 0.5, 2, 1]
OUT_KEYS = ("losses", "logits", "dopred", "att", "att_c", "att_h")
REF_OF = {"logits": "logits", "dopred": "dopred", "att": "att", "att_c": "c", "att_h": "h"}
_PROBLEMS = {}


# ------------------------------------------------------------------------------------------ machinery
def problem(name):
    """(shapes, batch, params, masks, c0, h0): (c0, h0) [B,R] f32 are the fp64 oracle's final state of another batch
    (seed 77) under the same parameters, in evaluate mode.  Computed once, shared, never changed."""
    if name not in _PROBLEMS:
        dims, scale = SHAPES[name]
        sh = util.shapes(dims)
        batch, params, masks = util.make_problem(sh, scale=scale)
        other, _, _ = util.make_problem(sh, seed=77, scale=scale)
        z = np.zeros((sh.B, sh.R))
        prev = state_ref.step(sh, params, other, None, None, z, z, backward=False)
        _PROBLEMS[name] = (sh, batch, params, masks, prev["c"][-1].astype(np.float32), prev["h"][-1].astype(np.float32))
    sh, batch, params, masks, c0, h0 = _PROBLEMS[name]
    return sh, dict(batch), params, masks, c0, h0


def hop_w(sh, w=HOP_W):
    return list(w)[:sh.H]


def counts(sh):
    return np.minimum(np.array([sh.S, 7, 3, 1, 5, sh.S, 2, 9], np.int32)[:sh.B], sh.S).astype(np.int32)


def put(m, batch, labelled=True, **kw):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"] if labelled else None, **kw)


def dev(a, dtype=torch.float32):
    t = (a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))).to(dtype).cuda()
    torch.cuda.synchronize()            # the upload ran on torch's stream: done before the ctx reads it
    return t


def narrowed(c0, h0, dtype):
    """(c0, h0) rounded to a 16-bit dtype, as the f32 values the device widens them to."""
    return tuple(torch.as_tensor(a).to(dtype).float().numpy() for a in (c0, h0))


DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def attach(m, c0, h0, dtype=torch.float32):
    """Upload (c0, h0) and attach them; the tensors are returned so that they outlive the launch."""
    tc, th = dev(c0, dtype), dev(h0, dtype)
    m.set_state(tc, th)
    assert m.batch_state
    return tc, th


def dev_step(m, w, out_grads=None, state_grads=None, graph=False):
    """One step on the resident batch: (outputs, parameter gradients)."""
    if graph:
        m.graph_step(f32(w))
    else:
        m.zero_grads()
        m.forward()
        m.backward(None if w is None else f32(w), out_grads=out_grads, state_grads=state_grads)
    return m.outputs(), m.get_grads()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_outputs(a, b, what=""):
    for k in OUT_KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what} {k}"


def assert_same_step(a, b, what=""):
    assert_same_outputs(a[0], b[0], what)
    same_bits(a[1], b[1])


def assert_close(got, ref, what, tol=TOL):
    e = util.rel_err(got, ref)
    print(f"{what}: rel_err {e:.2e} (max |ref| {np.max(np.abs(ref)):.2e})")
    assert np.max(np.abs(ref)) > 0, what
    assert e < tol, f"{what}: {e} >= {tol}"


def assert_outputs(outs, ref, what, tol=TOL):
    for k, r in REF_OF.items():
        assert_close(outs[k], ref[r], f"{what} {k}", tol)


def assert_grads(m_layouts, grads, ref, what):
    errs = grad_errs(grads, ref, m_layouts)
    bad = {k: v for k, v in errs.items() if not v < TOL}
    print(f"{what}: worst layer {max(errs.values()):.2e}")
    assert not bad, (what, bad)


def launches(m):
    return {n: v["launches"] for n, v in m.prof().items() if v["launches"]}


def tied_masks(sh, masks):
    one = dict(masks, x=np.ascontiguousarray(masks["x"][0]))
    return one, dict(masks, x=np.ascontiguousarray(np.broadcast_to(one["x"], (sh.H,) + one["x"].shape)))


# ------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("name,variant", [("SMALL", "train"), ("SMALL", "evaluate"), ("SMALL", "regions"),
                                          ("X196", "train"), ("B66", "evaluate"), ("EDGE", "f16"),
                                          ("SMALL", "bf16in")])
def test_forward_from_an_attached_state_against_the_reference(name, variant):
    sh, batch, params, masks, c0, h0 = problem(name)
    dtype = {"f16": torch.float16, "bf16in": torch.bfloat16}.get(variant, torch.float32)
    if dtype != torch.float32:
        c0, h0 = narrowed(c0, h0, dtype)
    m = make_model(sh, params, None if variant == "evaluate" else masks)
    kw, ref_kw = {}, {}
    if variant == "evaluate":
        m.evaluate()
    if variant == "regions":
        kw["regions"] = ref_kw["nreg"] = counts(sh)
    put(m, batch, **kw)
    keep = attach(m, c0, h0, dtype)
    m.forward()
    outs = m.outputs()
    cs, hs = m.state_tensors()
    torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(m.stream()))
    assert np.array_equal(bits(cs.cpu().numpy()), bits(outs["att_c"]))      # the views are the getters' rows
    assert np.array_equal(bits(hs.cpu().numpy()), bits(outs["att_h"]))
    m.close()
    ref = state_ref.step(sh, params, batch, None if variant == "evaluate" else masks, None, c0, h0, backward=False,
                         **ref_kw)
    assert_outputs(outs, ref, f"{name} {variant}")
    zero = state_ref.step(sh, params, batch, None if variant == "evaluate" else masks, None, 0 * c0, 0 * h0,
                          backward=False, **ref_kw)
    assert util.rel_err(zero["logits"], ref["logits"]) > 100 * TOL          # the state matters at this scale
    del keep


# ------------------------------------------------------------------------------------------ 2. backward
BACKWARD = [(n, "train") for n in ("SMALL", "M16", "EDGE", "X196", "B66")] + \
           [("SMALL", v) for v in ("tied", "question", "featgrad", "evaluate", "f16", "bf16in")] + \
           [("M16", "evaluate"), ("EDGE", "f16"), ("EDGE", "bf16in")]


@pytest.mark.parametrize("name,variant", BACKWARD)
def test_backward_leaves_the_state_gradient_against_the_reference(name, variant):
    sh, batch, params, masks, c0, h0 = problem(name)
    w = hop_w(sh)
    ref_masks, ref_kw, dtype = masks, {}, torch.float32
    m = make_model(sh, params, None if variant == "evaluate" else masks)
    if variant == "evaluate":
        m.evaluate()
        ref_masks = None
    elif variant == "tied":
        one, ref_masks = tied_masks(sh, masks)
        m.tie_feature_dropout()
        m.set_masks(one)
    elif variant == "featgrad":
        m.want_feature_grad()
        ref_kw["want_feats"] = True
    elif variant in ("f16", "bf16in"):      # 16-bit state inputs: the reference starts from the widened values
        dtype = torch.float16 if variant == "f16" else torch.bfloat16
        c0, h0 = narrowed(c0, h0, dtype)
    put(m, batch)
    keep = [attach(m, c0, h0, dtype)]
    if variant == "question":
        with torch.no_grad():
            q0 = question_ref.encoder_q(sh, torch.as_tensor(params["embed"]).double(),
                                        torch.as_tensor(params["rnn"]).double(), batch, masks).numpy().astype(np.float32)
        keep.append(dev(q0))
        m.set_question(keep[-1])
        ref_kw["q"] = q0
    outs, grads = dev_step(m, w)
    d_c0, d_h0 = m.state_grad()
    tc, th = m.state_grad_tensors()
    torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(m.stream()))
    assert np.array_equal(bits(tc.cpu().numpy()), bits(d_c0)) and np.array_equal(bits(th.cpu().numpy()), bits(d_h0))
    dq = m.question_grad() if variant == "question" else None
    dX = m.feature_grad() if variant == "featgrad" else None
    layouts = {g: m.layout(g) for g in (("mult",) if variant == "question" else ("embed", "rnn", "mult"))}
    m.close()
    ref = state_ref.step(sh, params, batch, ref_masks, w, c0, h0, **ref_kw)
    what = f"{name} {variant}"
    assert_outputs(outs, ref, what)
    assert_close(d_c0, ref["d_c0"], what + " d_c0")
    assert_close(d_h0, ref["d_h0"], what + " d_h0")
    assert_grads(layouts, grads, ref, what)
    if dq is not None:
        assert_close(dq, ref["g_q"], what + " dq")
        assert not grads["embed"].any() and not grads["rnn"].any()
    if dX is not None:
        assert_close(np.asarray(dX).reshape(ref["g_feats"].shape), ref["g_feats"], what + " dX")
    del keep


def test_backward_in_bf16_mode_against_the_emulated_reference():
    """bf16 mode: d_c0, d_h0, c, h, logits and every layer slice of the three gradient groups, each at its own derived
    bar (tests/test_gpu_bf16.py::run's part 1, tensor by tensor)."""
    sh, batch, params, masks, c0, h0 = problem("SMALL")
    w = hop_w(sh)
    m = make_model(sh, params, masks, dtype="bf16")
    put(m, batch)
    keep = attach(m, c0, h0)
    outs, grads = dev_step(m, w)
    layouts = {g: m.layout(g) for g in ("embed", "rnn", "mult")}
    d_c0, d_h0 = m.state_grad()
    m.close()

    def tensors(res, g):
        out = {k: np.asarray(res[k]) for k in ("d_c0", "d_h0", "c", "h", "logits")}
        for grp in layouts:
            for lname, sl in util.layer_slices(layouts[grp]):
                out[lname] = np.asarray(g[grp][sl])
        return out

    got = tensors({"d_c0": d_c0, "d_h0": d_h0, "c": outs["att_c"], "h": outs["att_h"], "logits": outs["logits"]}, grads)
    of_ref = lambda r: tensors(r, {grp: r["g_" + grp] for grp in layouts})
    with RT.bf16_emulation():
        emu = of_ref(state_ref.step(sh, params, batch, masks, w, c0, h0, bf16=True))
    nudged = []
    for nudge in NUDGES:
        with RT.bf16_emulation(nudge):
            nudged.append(of_ref(state_ref.step(sh, params, batch, masks, w, c0, h0, bf16=True)))
    err = lambda a, b: float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    bad, ratio = {}, 0.0
    assert {"classifier.attlstm.h2h.weight", "attbymemory.linear.weight", "q_embed.h_proj.weight"} <= set(got)     # the three that read h0 from slot 0
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
    del keep


@pytest.mark.parametrize("name", ["SMALL", "EDGE"])
def test_no_active_hop_gives_exact_zeros(name):
    sh, batch, params, masks, c0, h0 = problem(name)
    m = make_model(sh, params, masks)
    put(m, batch)
    keep = attach(m, c0, h0)
    dev_step(m, hop_w(sh))
    assert all(g.any() for g in m.state_grad())
    dev_step(m, [0.0] * sh.H)
    for g in m.state_grad():
        assert g.shape == (sh.B, sh.R) and not bits(g).any()        # +0 everywhere, not the step before's value
    m.close()
    del keep


# ------------------------------------------------------------------------------------------ 3. incoming gradients
def state_G(sh, seed=5):
    rng = np.random.default_rng(seed)
    return {"h": (rng.normal(size=(sh.H, sh.B, sh.R)) / sh.B).astype(np.float32),
            "c_last": (rng.normal(size=(sh.B, sh.R)) / sh.B).astype(np.float32),
            "logits": (rng.normal(size=(sh.H, sh.B, sh.K)) / sh.B).astype(np.float32)}


@pytest.mark.parametrize("name,which", [("SMALL", "h"), ("SMALL", "c_last"), ("SMALL", "both+logits"),
                                        ("SMALL", "ext_only"), ("EDGE", "both+logits"), ("M16", "both+logits"),
                                        ("EDGE", "both+logits/f16"), ("SMALL", "h/bf16")])
def test_incoming_state_gradients_against_the_reference(name, which):
    """F = <G_h, hs> + <G_c, cs[-1]> (+ <G_l, logits>): its gradients at the states are the G themselves.
    ext_only: no hop_w, a batch without labels; trailing zero hop weights elsewhere, so every hop is active by the
    external terms' rule alone."""
    sh, batch, params, masks, c0, h0 = problem(name)
    which, _, dt = which.partition("/")
    dtype = DT[dt or "f32"]
    if dt:                                  # a 16-bit attached state under the incoming gradients
        c0, h0 = narrowed(c0, h0, dtype)
    G = state_G(sh)
    use = {"h": ("h",), "c_last": ("c_last",), "both+logits": ("h", "c_last", "logits"), "ext_only": ("h", "c_last")}[which]
    labelled = which != "ext_only"
    w = (hop_w(sh, [3, 0, 0]) if sh.H > 1 else hop_w(sh)) if labelled else None
    m = make_model(sh, params, masks)
    put(m, batch, labelled)
    keep = attach(m, c0, h0, dtype)
    sg = {k: dev(G[k]) for k in use if k != "logits"}
    og = {"logits": dev(G["logits"])} if "logits" in use else None
    outs, grads = dev_step(m, w, og, sg)
    d_c0, d_h0 = m.state_grad()
    layouts = {g: m.layout(g) for g in ("embed", "rnn", "mult")}
    m.close()
    F = state_ref.linear_F(G_l=G["logits"] if "logits" in use else None, G_h=G["h"] if "h" in use else None,
                           G_c_last=G["c_last"] if "c_last" in use else None)
    ref = state_ref.step(sh, params, batch if labelled else dict(batch, labels=None), masks, w, c0, h0, F=F)
    what = f"{name} {which}"
    assert_outputs(outs, ref, what)
    assert_close(d_c0, ref["d_c0"], what + " d_c0")
    assert_close(d_h0, ref["d_h0"], what + " d_h0")
    assert_grads(layouts, grads, ref, what)
    del keep, sg, og


def test_incoming_state_gradients_without_an_attached_state():
    """rau_backward_state on a detached batch: the gradients enter, none is handed out."""
    sh, batch, params, masks, _, _ = problem("SMALL")
    G = state_G(sh)
    m = make_model(sh, params, masks)
    put(m, batch)
    sg = {k: dev(G[k]) for k in ("h", "c_last")}
    _, grads = dev_step(m, hop_w(sh), None, sg)
    assert m._lib.rau_state_grad_dev(m._h, None, None) == STATE
    layouts = {g: m.layout(g) for g in ("embed", "rnn", "mult")}
    m.close()
    z = np.zeros((sh.B, sh.R))
    ref = state_ref.step(sh, params, batch, masks, hop_w(sh), z, z, F=state_ref.linear_F(G_h=G["h"], G_c_last=G["c_last"]))
    assert_grads(layouts, grads, ref, "detached")
    del sg


# ------------------------------------------------------------------------------------------ 4. truncated BPTT
def test_two_chained_contexts_equal_four_hops():
    """Evaluate mode.  Context A runs hops 1-2, context B attaches A's final state (device pointers: A's own
    rau_state_dev rows) and runs hops 3-4; B's d_c0 / d_h0 enter A's rau_backward_state as d_c_last and the last row
    of d_h.  The summed gradients equal the reference's H = 4 gradients; att, c, h equal an H = 4 context's bits."""
    sh4, batch, params, _, c0, h0 = problem("H4")
    c0, h0 = narrowed(c0, h0, torch.float16)          # the chain's own initial state arrives as float16
    sh2 = problem("H2")[0]
    w = hop_w(sh4)
    A, B, W = (make_model(s, params) for s in (sh2, sh2, sh4))
    for m in (A, B, W):
        m.evaluate()
        put(m, batch)
    keep = attach(A, c0, h0, torch.float16), attach(W, c0, h0, torch.float16)
    whole = dev_step(W, w)
    A.zero_grads(); A.forward()
    a_out = A.outputs()
    ca, ha = A.state_tensors()
    A.sync()                                 # B's stream reads A's rows: A's forward is done
    B.set_state(ca[-1], ha[-1])
    b_out, b_grads = dev_step(B, w[2:])
    dcb, dhb = B.state_grad_tensors()
    B.sync()                                 # ... and A's stream reads B's gradient
    d_h = torch.zeros(sh2.H, sh2.B, sh2.R, device="cuda")
    d_h[-1] = dhb
    d_c = dcb.clone()
    torch.cuda.synchronize()
    A.backward(f32(w[:2]), state_grads={"h": d_h, "c_last": d_c})
    a_grads = A.get_grads()
    d_c0, d_h0 = A.state_grad()
    whole_d = W.state_grad()
    layouts = {g: W.layout(g) for g in ("embed", "rnn", "mult")}
    for m in (A, B, W):
        m.close()
    for k in ("att", "att_c", "att_h", "logits", "dopred"):
        assert np.array_equal(bits(np.concatenate([a_out[k], b_out[k]])), bits(whole[0][k])), k
    ref = state_ref.step(sh4, params, batch, None, w, c0, h0)
    summed = {g: a_grads[g] + b_grads[g] for g in a_grads}
    assert_grads(layouts, summed, ref, "A + B")
    assert_grads(layouts, whole[1], ref, "H = 4")
    assert_close(d_c0, ref["d_c0"], "chain d_c0"); assert_close(d_h0, ref["d_h0"], "chain d_h0")
    assert_close(whole_d[0], ref["d_c0"], "H = 4 d_c0"); assert_close(whole_d[1], ref["d_h0"], "H = 4 d_h0")
    del keep


def test_carry_state_runs_more_hops_than_the_context_has():
    """carry_state(): forward, carry, forward again is hops H+1 .. 2H -- against the reference's run of 2H hops."""
    sh2, batch, params, _, _, _ = problem("H2")
    sh4 = problem("H4")[0]
    m = make_model(sh2, params)
    m.evaluate()
    put(m, batch)
    m.forward()
    first = m.outputs()
    m.carry_state()
    assert m.batch_state
    m.forward()
    second = m.outputs()
    m.close()
    z = np.zeros((sh4.B, sh4.R))
    ref = state_ref.step(sh4, params, batch, None, None, z, z, backward=False)
    for k, r in REF_OF.items():
        assert_close(np.concatenate([first[k], second[k]]), ref[r], "carried " + k)


# ------------------------------------------------------------------------------------------ 5. identities
@pytest.mark.parametrize("name", ["SMALL", "M16", "EDGE"])
def test_an_all_zero_state_gives_the_detached_forward(name):
    sh, batch, params, masks, c0, h0 = problem(name)
    m = make_model(sh, params, masks)
    put(m, batch)
    detached = dev_step(m, hop_w(sh))
    keep = attach(m, 0 * c0, 0 * h0)
    zero = dev_step(m, hop_w(sh))
    assert_same_outputs(zero[0], detached[0], name)
    # hop 0 takes the other hops' branch then: the parameter gradients agree at the bar, not by rule in their bits
    assert util.rel_err(zero[1]["mult"], detached[1]["mult"]) < TOL
    m.close()
    del keep


@pytest.mark.parametrize("name", ["SMALL", "EDGE"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_16_bit_states_give_the_bits_of_the_widened_f32_state(name, dt):
    """EDGE: n R / 4 = 5 quads, so the 16-bit form's last quad is the odd one (one 8-byte load)."""
    sh, batch, params, masks, c0, h0 = problem(name)
    wide = narrowed(c0, h0, DT[dt])
    assert not np.array_equal(wide[0], c0) and (sh.B * sh.R // 4) % 2 == (1 if name == "EDGE" else 0)
    m = make_model(sh, params, masks)
    put(m, batch)
    keep = attach(m, *wide)
    a = dev_step(m, hop_w(sh))
    da = m.state_grad()
    keep16 = attach(m, *wide, DT[dt])
    assert keep16[0].dtype == DT[dt]
    b = dev_step(m, hop_w(sh))
    db = m.state_grad()
    m.close()
    assert_same_step(a, b, f"{name} {dt}")
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(da, db))
    del keep, keep16


@pytest.mark.parametrize("how", ["clear", "set_batch", "set_batch_dev", "use_batch", "set_batch_size"])
def test_detached_again_is_never_attached(how):
    """Attach, step, detach (by the call or by rule), step: every output and gradient of a never-attached step, and
    the profile's launch names and counts."""
    sh, batch, params, masks, c0, h0 = problem("SMALL")
    w = hop_w(sh)
    m = make_model(sh, params, masks)
    put(m, batch)
    m.prof_enable()
    never = dev_step(m, w)
    never_l = launches(m)
    m.prof_enable(False)
    assert "state_attach" not in never_l and "state_grad_finish" not in never_l
    if how == "use_batch":
        m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    keep = attach(m, c0, h0)
    with_state = dev_step(m, w)
    assert not np.array_equal(with_state[0]["logits"], never[0]["logits"])
    if how == "clear":
        m.clear_state()
    elif how == "set_batch":
        put(m, batch)
    elif how == "set_batch_dev":
        x = dev(batch["feats"])
        m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"])
    elif how == "use_batch":
        m.use_batch(1)
    else:
        m.set_batch_size(sh.B - 1)
        assert not m.batch_state
        m.set_batch_size(sh.B)
        m.set_masks(masks)
        put(m, batch)
    assert not m.batch_state
    m.prof_reset()
    m.prof_enable()
    again = dev_step(m, w)
    assert launches(m) == never_l
    m.prof_enable(False)
    assert_same_step(again, never, how)
    assert m._lib.rau_state_grad_dev(m._h, None, None) == STATE
    if how == "use_batch":                                            # ... and back: the state did not stay behind
        m.use_batch(0)
        assert not m.batch_state
        assert_same_step(dev_step(m, w), never, "slot 0 again")
    m.close()
    del keep


def test_one_launch_more_per_pass_with_a_state():
    """The attached step: the detached step's launches plus state_grad_finish; the attach is one state_attach."""
    sh, batch, params, masks, c0, h0 = problem("SMALL")
    m = make_model(sh, params, masks)
    put(m, batch)
    m.prof_enable()
    dev_step(m, hop_w(sh))
    detached = launches(m)
    m.prof_reset()
    keep = attach(m, c0, h0)
    assert launches(m) == {"state_attach": 1}
    m.prof_reset()
    dev_step(m, hop_w(sh))
    got = launches(m)
    assert got.pop("state_grad_finish") == 1
    # hop 0 forms its three products towards prev_h: with M != R that is three small GEMMs more
    assert got.pop("small_gemm") == detached.pop("small_gemm") + 3
    assert got == detached
    m.close()
    del keep


def test_null_state_gradients_are_backward_ext():
    sh, batch, params, masks, c0, h0 = problem("SMALL")
    G = state_G(sh)
    w = f32(hop_w(sh))
    m = make_model(sh, params, masks)
    put(m, batch)
    keep = attach(m, c0, h0)
    og = dev(G["logits"])
    g = L.RauOutGrads(og.data_ptr(), None, None)
    m.prof_enable()
    results = []
    for sg in ("ext", None, L.RauStateGrads(None, None)):
        m.prof_reset()
        m.zero_grads(); m.forward()
        if sg == "ext":
            L.check(m._lib.rau_backward_ext(m._h, w.ctypes.data, None, None, None, C.byref(g)))
        else:
            L.check(m._lib.rau_backward_state(m._h, w.ctypes.data, None, None, None, C.byref(g),
                                              None if sg is None else C.byref(sg)))
        results.append((m.get_grads(), m.state_grad(), launches(m)))
    m.close()
    for got in results[1:]:
        same_bits(got[0], results[0][0])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[1], results[0][1]))
        assert got[2] == results[0][2]
    del keep, og


@pytest.mark.parametrize("name", ["SMALL", "M16"])
def test_two_identical_steps_give_identical_bits(name):
    sh, batch, params, masks, c0, h0 = problem(name)
    G = state_G(sh)
    m = make_model(sh, params, masks)
    put(m, batch)
    keep = attach(m, c0, h0)
    sg = {k: dev(G[k]) for k in ("h", "c_last")}
    a = dev_step(m, hop_w(sh), None, sg)
    da = m.state_grad()
    m.zero_grads()                                   # rau_zero_grads does not touch the state gradient
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(m.state_grad(), da))
    b = dev_step(m, hop_w(sh), None, sg)
    db = m.state_grad()
    m.close()
    assert_same_step(a, b, name)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(da, db))
    del keep, sg


# ------------------------------------------------------------------------------------------ 6. captured steps
@pytest.mark.parametrize("name", ["SMALL", "M16"])
def test_captured_steps_with_and_without_a_state(name):
    sh, batch, params, masks, c0, h0 = problem(name)
    w = hop_w(sh)
    m = make_model(sh, params, masks)
    twin = make_model(sh, params, masks)             # the eager twin
    put(m, batch); put(twin, batch)
    dtype = torch.bfloat16 if name == "M16" else torch.float32     # M16: the states arrive as bfloat16
    states = [(c0, h0), (0.5 * c0, -h0)]
    if name == "M16":
        states = [narrowed(*s, dtype) for s in states]
    eager, eager_d = [], []
    for s in states:
        keep = attach(twin, *s, dtype)
        eager.append(dev_step(twin, w))
        eager_d.append(twin.state_grad())
    twin.clear_state()
    eager_none = dev_step(twin, w)
    twin.close()
    # one capture, another state per replay: the graph holds the rows' address, a replay reads what is attached now
    for i in (0, 1, 0):
        keep = attach(m, *states[i], dtype)
        assert_same_step(dev_step(m, w, graph=True), eager[i], f"replay {i}")
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(m.state_grad(), eager_d[i])), i
    # the key's state member selects its own graph: no state, state, no state
    for i in (None, 1, None):
        if i is None:
            m.clear_state()
            assert_same_step(dev_step(m, w, graph=True), eager_none, "no state")
            assert m._lib.rau_state_grad_dev(m._h, None, None) == STATE
        else:
            keep = attach(m, *states[i], dtype)
            assert_same_step(dev_step(m, w, graph=True), eager[i], "state")
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(m.state_grad(), eager_d[i]))
    m.close()
    del keep


# ------------------------------------------------------------------------------------------ 7. errors
def test_refusals_change_nothing():
    sh, batch, params, masks, c0, h0 = problem("SMALL")
    m = make_model(sh, params, masks)
    lib, h = m._lib, m._h
    n = c0.size
    t = dev(np.concatenate([c0.reshape(-1), h0.reshape(-1), np.zeros(4, np.float32)]))
    pc, ph = C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr() + 4 * n)
    p, q = C.c_void_p(), C.c_void_p()
    assert lib.rau_set_state_dev(h, pc, ph, 0) == STATE                                # no resident batch
    assert b"batch" in lib.rau_last_error()
    assert lib.rau_state_dev(h, C.byref(p), C.byref(q)) == STATE                       # no forward to read
    put(m, batch)
    detached = dev_step(m, hop_w(sh))
    m.prof_enable()
    assert lib.rau_set_state_dev(h, pc, None, 0) == INVALID                            # exactly one NULL pointer
    assert lib.rau_set_state_dev(h, None, ph, 0) == INVALID
    assert lib.rau_set_state_dev(h, C.c_void_p(t.data_ptr() + 4), ph, 0) == INVALID    # misaligned
    assert b"aligned" in lib.rau_last_error()
    for ty in (4, 5, 3, -1, 6):                                                        # e4m3, e5m2, reserved, unknown
        assert lib.rau_set_state_dev(h, pc, ph, ty) == INVALID, ty
    bad = L.RauStateGrads(t.data_ptr() + 4, None)
    m.forward()
    assert lib.rau_backward_state(h, f32(hop_w(sh)).ctypes.data, None, None, None, None, C.byref(bad)) == INVALID
    assert launches(m).get("state_attach") is None and not m.batch_state               # nothing was launched
    m.prof_enable(False)
    assert_same_step(dev_step(m, hop_w(sh)), detached, "after the refusals")           # still detached
    # ... and with a state attached (here as float16) the refusals leave THAT state in force
    t16 = dev(np.concatenate([c0.reshape(-1), h0.reshape(-1)]), torch.float16)
    m.set_state(t16[:n].view(sh.B, sh.R), t16[n:].view(sh.B, sh.R))
    attached = dev_step(m, hop_w(sh))
    assert lib.rau_set_state_dev(h, pc, None, 0) == INVALID
    assert lib.rau_set_state_dev(h, pc, ph, 4) == INVALID
    assert m.batch_state
    assert_same_step(dev_step(m, hop_w(sh)), attached, "after the refusals, attached")
    # the gradient: not before a backward of the current forward
    m.forward()
    assert lib.rau_state_grad_dev(h, C.byref(p), C.byref(q)) == STATE
    host = np.empty_like(c0)
    assert lib.rau_get_state_grad(h, C.c_void_p(host.ctypes.data), None) == STATE
    m.backward(f32(hop_w(sh)))
    assert lib.rau_state_grad_dev(h, C.byref(p), C.byref(q)) == 0 and p.value and q.value
    assert lib.rau_get_state_grad(h, C.c_void_p(host.ctypes.data), None) == 0           # either half may be NULL
    # attaching again (other values, or the same): what the last backward left is not THIS state's gradient
    m.set_state(t[:n].view(sh.B, sh.R), t[n:2 * n].view(sh.B, sh.R))
    assert lib.rau_state_grad_dev(h, C.byref(p), C.byref(q)) == STATE
    assert lib.rau_get_state_grad(h, C.c_void_p(host.ctypes.data), None) == STATE
    dev_step(m, hop_w(sh))
    assert lib.rau_state_grad_dev(h, C.byref(p), C.byref(q)) == 0
    put(m, batch)                                                                       # ... nor another batch's
    m.set_state(t[:n].view(sh.B, sh.R), t[n:2 * n].view(sh.B, sh.R))
    assert lib.rau_state_grad_dev(h, C.byref(p), C.byref(q)) == STATE
    dev_step(m, hop_w(sh))
    m.clear_state()
    assert lib.rau_state_grad_dev(h, C.byref(p), C.byref(q)) == STATE
    m.set_state(t[:n].view(sh.B, sh.R), t[n:2 * n].view(sh.B, sh.R))
    assert lib.rau_state_grad_dev(h, C.byref(p), C.byref(q)) == STATE
    # a forward that ran before an attach (or a detach) has no backward
    hp = f32(hop_w(sh))
    m.forward()
    m.set_state(t[:n].view(sh.B, sh.R), t[n:2 * n].view(sh.B, sh.R))
    assert lib.rau_backward(h, hp.ctypes.data) == STATE
    m.forward()
    m.clear_state()
    assert lib.rau_backward(h, hp.ctypes.data) == STATE
    m.close()


# ------------------------------------------------------------------------------------------ 8. autograd.step
@pytest.mark.parametrize("name,dt", [("SMALL", "f32"), ("M16", "f32"), ("M16", "f16")])
def test_autograd_step_with_a_state_and_a_torch_head_on_h(name, dt):
    """A torch Linear head on h' of every hop and a term on c_last, plus hop_w's criterion: c0.grad, h0.grad, the
    head's own gradients and the parameter gradients against the fp64 restatement.  f16: the state tensors are
    float16, and so are their .grad: the f32 gradient rounded to nearest, at most 2^-11 of an element's size away --
    the bar for those two is TOL + 2^-11 (nothing is below float16's normal range at this scale: asserted)."""
    from rau_vqa_amd import autograd
    sh, batch, params, masks, c0, h0 = problem(name)
    dtype = DT[dt]
    if dt != "f32":
        c0, h0 = narrowed(c0, h0, dtype)
    rng = np.random.default_rng(21)
    W0 = (0.4 * rng.normal(size=(5, sh.R))).astype(np.float32)
    tgt = rng.integers(0, 5, size=(sh.B,))
    w = hop_w(sh)

    def objective(scores, dps, atts, cs, hs, Wt, y):
        head = sum(torch.nn.functional.cross_entropy(hh @ Wt.T, y) for hh in hs)
        return head + 0.3 * (cs[-1] ** 2).sum() / sh.B + 0.05 * sum(d.mean() for d in dps)

    m = make_model(sh, params, masks)
    put(m, batch)
    tc = dev(c0, dtype).requires_grad_(True)
    th = dev(h0, dtype).requires_grad_(True)
    Wd = dev(W0).requires_grad_(True)
    m.set_state(tc.detach(), th.detach())
    m.zero_grads()
    logits, dopred, attprob, hs, c_last = autograd.step(m, hop_w=f32(w), state=(tc, th), return_state=True)
    assert tuple(hs.shape) == (sh.H, sh.B, sh.R) and tuple(c_last.shape) == (sh.B, sh.R)
    loss = objective(list(logits), list(dopred), list(attprob), [None] * (sh.H - 1) + [c_last], list(hs), Wd,
                     torch.as_tensor(tgt).cuda())
    loss.backward()
    assert tc.grad.dtype == dtype and th.grad.dtype == dtype
    got = {"c0": tc.grad.float().cpu().numpy(), "h0": th.grad.float().cpu().numpy(), "W": Wd.grad.cpu().numpy()}
    grads = m.get_grads()
    layouts = {g: m.layout(g) for g in ("embed", "rnn", "mult")}
    # the default call on the same attached batch still returns three tensors, with the same bits.  (It also makes
    # torch allocate once more while the context lives: the caching allocator then retires the events it recorded on
    # the context's stream for the gradient tensors, before close() destroys that stream.)
    out3 = autograd.step(m, hop_w=f32(w))
    assert len(out3) == 3 and torch.equal(out3[0], logits) and torch.equal(out3[2], attprob)
    torch.cuda.synchronize()
    m.close()

    Wt = torch.as_tensor(W0, dtype=torch.float64).requires_grad_(True)
    F = lambda s, d, a, cs, hs_: objective(s, d, a, cs, hs_, Wt, torch.as_tensor(tgt))
    ref = state_ref.step(sh, params, batch, masks, w, c0, h0, F=F)
    tol = TOL if dt == "f32" else TOL + 2.0 ** -11
    if dt == "f16":     # rel_err is a max-norm figure: the rounding of the largest element bounds it, given no underflow
        assert all(np.abs(ref[k]).max() > 2.0 ** -14 for k in ("d_c0", "d_h0"))
    assert_close(got["c0"], ref["d_c0"], name + " c0.grad", tol)
    assert_close(got["h0"], ref["d_h0"], name + " h0.grad", tol)
    assert_close(got["W"], Wt.grad.numpy(), name + " head weight gradient")
    assert_grads(layouts, grads, ref, name + " autograd")
