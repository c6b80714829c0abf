"""Custom objectives on the GPU (rau_outputs_dev, rau_backward_ext, ext_grad.hip, rau_vqa_amd/autograd.py): the
step-level backward from caller-supplied gradients at logits, do_pred and attprob.

The oracle is tests/ext_ref.py (ref_torch's loop restated in fp64 autograd: merge_ref.step's objective, att_ref.step's
attention term, plus a callable F on the outputs), the machinery tests/test_gpu_select.py's and
tests/test_gpu_merged.py's: the committed problems under their explicit masks, make_model, grad_errs, same_bits,
check_gates, TOL = 1e-4 per layer slice.

Section 1 uses a LINEAR functional F = sum_h <G_l[h], logits_h> + <G_d[h], dopred_h> + <G_a[h], att_h> with fixed
seeded G of the size of a CE gradient (entries about 1/n): its gradients at the outputs are the G themselves,
whatever the device computed in the forward.  Section 2 states built-in terms as external gradients with the numpy
functions of rau_vqa_amd/joint.py, which are written in the device's operation order, and asserts equal BITS.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from rau_vqa_amd import joint
from tests import att_ref, ext_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_merged import check_gates
from tests.test_gpu_select import (GROUPS, INVALID, STATE, TOL, check_argmax, f32, grad_errs, make_model, problem,
                                   same_bits, targets)

pytestmark = pytest.mark.gpu

COUNTS8 = np.array([12, 7, 3, 1, 5, 12, 2, 9], np.int32)     # region counts of an 8-sample batch at S = 12


# ------------------------------------------------------------------------------------------ machinery
def seeded_G(H, n, K, S, seed=5):
    """G_l [H,n,K], G_d [H,n], G_a [H,n,S] float32, entries about 1/n."""
    rng = np.random.default_rng(seed)
    return {"logits": (rng.normal(size=(H, n, K)) / n).astype(np.float32),
            "dopred": (rng.normal(size=(H, n)) / n).astype(np.float32),
            "attprob": (rng.normal(size=(H, n, S)) / n).astype(np.float32)}


def pick(G, which):
    """The entries of G named by the letters of `which` (l, d, a)."""
    return {k: G[k] for k in G if k[0] in which}


def linear_F(G):
    return ext_ref.linear_F(G.get("logits"), G.get("dopred"), G.get("attprob"))


def on_device(G):
    out = {k: torch.as_tensor(np.ascontiguousarray(v, np.float32)).cuda() for k, v in G.items()}
    torch.cuda.synchronize()     # the uploads ran on torch's stream: done before the ctx's stream reads them
    return out


def ptr(a):
    return None if a is None else a.ctypes.data


def raw_ext(m, hop_w, select_w=None, att_w=None, merge_w=None, dev=None, struct=True):
    """rau_backward_ext through ctypes: the return code.  dev: device tensors by name; struct False passes g = NULL."""
    dev = dev or {}
    g = L.RauOutGrads(*(dev[k].data_ptr() if k in dev else None for k in ("logits", "dopred", "attprob")))
    ws = [None if w is None else f32(w) for w in (hop_w, select_w, att_w, merge_w)]
    return m._lib.rau_backward_ext(m._h, *(ptr(w) for w in ws), C.byref(g) if struct else None)


def ext_step(m, G, hop_w=None, select_w=None, att_w=None, merge_w=None):
    """zero_grads + forward + backward(out_grads=G) on the resident batch: the gradients."""
    m.zero_grads()
    m.forward()
    dev = on_device(G)
    m.backward(None if hop_w is None else f32(hop_w), select_w, att_w, merge_w, out_grads=dev)
    got = m.get_grads()          # synchronises the ctx's stream: dev has been read
    return got


def assert_within(got, ref, layouts, what=""):
    errs = grad_errs(got, ref, layouts)
    worst = max(errs, key=errs.get)
    print(f"{what}: largest error {errs[worst]:.1e} ({worst})")
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"{what}: relative errors above {TOL}: {bad}"


def put(m, batch, labelled=True, **kw):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"] if labelled else None, **kw)


def linear_parity(dims_name, which, hop_w, labelled=True, evaluate=False):
    sh, batch, params, masks = problem(dims_name)
    m = make_model(sh, params, None if evaluate else masks)
    if evaluate:
        m.evaluate()
    put(m, batch, labelled)
    G = pick(seeded_G(sh.H, sh.B, sh.K, sh.S), which)
    got = ext_step(m, G, hop_w)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = ext_ref.step(sh, params, batch if labelled else dict(batch, labels=None), None if evaluate else masks,
                       hop_w, F=linear_F(G))
    assert_within(got, ref, layouts, f"{dims_name} {which}")
    return got, ref


# ------------------------------------------------------------------------------------------ 1. linear functional
@pytest.mark.parametrize("which", ["l", "d", "a"])
def test_each_gradient_alone_against_the_oracle(which):
    got, ref = linear_parity("SMALL", which, [3, 3, 3])
    plain = ext_ref.step(*_small_args(), [3, 3, 3])
    assert any(util.rel_err(ref["g_" + k], plain["g_" + k]) > 1e-3 for k in GROUPS)   # F is at work in the oracle


def _small_args():
    sh, batch, params, masks = problem("SMALL")
    return sh, params, batch, masks


@pytest.mark.parametrize("dims_name,hop_w", [("SMALL", [3, 3, 3]), ("EDGE", [1]), ("MEDIUM", [2, 2])])
def test_all_three_gradients_against_the_oracle(dims_name, hop_w):
    linear_parity(dims_name, "lda", hop_w)


def test_external_only_on_a_batch_without_labels():
    linear_parity("SMALL", "lda", None, labelled=False)
    linear_parity("SMALL", "d", None, labelled=False)      # no d_logits: dl is written as zeros, never read


def test_evaluate_mode():
    linear_parity("SMALL", "lda", [3, 3, 3], evaluate=True)


def test_together_with_every_built_in_term():
    sh, batch, params, masks = problem("SMALL")
    hop_w, select_w, att_w, merge_w = [3, 0.5, 2], [0.7, 0.4, 1.3], [0.5, 3.0, 1.5], [0.7, 1.3]
    fwd = ext_ref.step(sh, params, batch, masks, hop_w, backward=False)
    t = att_ref.targets(fwd["att"])
    assert att_ref.check(fwd["att"], t)
    m = make_model(sh, params, masks)
    put(m, batch, att_targets=t)
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    got = ext_step(m, G, hop_w, f32(select_w), f32(att_w), f32(merge_w))
    check_gates(m, fwd, sh.H)
    t_gt = targets(check_argmax(m, fwd), batch)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = ext_ref.step(sh, params, batch, masks, hop_w, merge_w, select_w, t_gt, F=linear_F(G), att_w=att_w, att_t=t)
    assert_within(got, ref, layouts, "all terms")


def test_batch_of_5_in_a_context_of_capacity_8():
    """Dense strides at n, not at the capacity: every G is [H, 5, ..]."""
    sh, batch, params, masks = problem("SMALL")
    n = 5
    sh5 = dataclasses.replace(sh, B=n)
    b5 = {"feats": batch["feats"][:n], "tokens": np.ascontiguousarray(batch["tokens"][:, :n]),
          "lens": batch["lens"][:n], "labels": batch["labels"][:n]}
    m5k = {k: np.ascontiguousarray(v[:, :n]) for k, v in masks.items()}
    m = make_model(sh, params, masks)
    m.set_batch_size(n)
    m.set_masks(m5k)
    put(m, b5)
    G = seeded_G(sh.H, n, sh.K, sh.S)
    got = ext_step(m, G, [3, 3, 3])
    lg, dp, at = m.output_tensors()
    assert tuple(lg.shape) == (sh.H, n, sh.K) and tuple(dp.shape) == (sh.H, n) and tuple(at.shape) == (sh.H, n, sh.S)
    assert np.array_equal(lg.cpu().numpy(), m.logits()) and np.array_equal(dp.cpu().numpy(), m.dopred())
    assert np.array_equal(at.cpu().numpy(), m.attention())
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = ext_ref.step(sh5, params, b5, m5k, [3, 3, 3], F=linear_F(G))
    assert_within(got, ref, layouts, "n = 5 of 8")


def test_region_counts_at_a_pitched_S():
    """S = 13: pitch 16 != S, and positions behind a count.  What G_a holds there is never read."""
    sh = util.shapes(util.SMALL, S=13)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    nreg = np.array([13, 7, 3, 1, 5, 13, 2, 9], np.int32)
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    m = make_model(sh, params, masks)
    put(m, batch, regions=nreg)
    got = ext_step(m, G, [3, 3, 3])
    at = m.output_tensors()[2]
    assert at.stride() == (sh.B * 16, 16, 1) and np.array_equal(at.cpu().numpy(), m.attention())
    live = np.arange(sh.S)[None, :] < nreg[:, None]
    Gz = dict(G, attprob=np.where(live[None], G["attprob"], np.float32(0)).astype(np.float32))
    assert not np.array_equal(Gz["attprob"], G["attprob"])
    same_bits(ext_step(m, Gz, [3, 3, 3]), got)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = ext_ref.step(sh, params, batch, masks, [3, 3, 3], F=linear_F(G), nreg=nreg)
    assert_within(got, ref, layouts, "S = 13 with counts")


# ------------------------------------------------------------------------------------------ 2. bit for bit
def builtin(m, name, *ws):
    """A built-in backward entry point through ctypes (None is NULL): the return code."""
    arrs = [None if w is None else f32(w) for w in ws]      # alive across the call
    return getattr(m._lib, name)(m._h, *(ptr(a) for a in arrs))


def builtin_step(m, name, *ws):
    m.zero_grads()
    m.forward()
    assert builtin(m, name, *ws) == 0
    return m.get_grads()


def test_attention_supervision_stated_as_an_external_gradient_gives_the_same_bits():
    sh, batch, params, masks = problem("SMALL")
    hop_w, select_w, att_w = [3, 0.5, 2], [0.7, 0, 1.3], [0.5, 3.0, 1.5]
    m = make_model(sh, params, masks)
    put(m, batch, regions=COUNTS8)
    m.forward()
    t = att_ref.targets(m.attention().astype(np.float64) + 1e-3, COUNTS8)    # any map with t > 0 below the counts
    for b, nb in enumerate(COUNTS8):
        t[b, nb:] = 7.0                                                     # behind the counts: to be ignored
    put(m, batch, regions=COUNTS8, att_targets=t)
    base = builtin_step(m, "rau_backward_att", hop_w, select_w, att_w)
    m.zero_grads()
    m.forward()
    d_att = joint.att_ce_grad(m.attention(), t, f32(att_w), COUNTS8)
    assert d_att.dtype == np.float32 and np.any(d_att != 0)
    dev = on_device({"attprob": d_att})
    assert raw_ext(m, hop_w, select_w, None, None, dev) == 0
    same_bits(m.get_grads(), base)
    m.close()


def test_selection_bce_stated_as_an_external_gradient_gives_the_same_bits():
    sh, batch, params, masks = problem("SMALL")
    hop_w, select_w = [3, 0.5, 2], [0.7, 0, 1.3]
    m = make_model(sh, params, masks)
    put(m, batch)
    base = builtin_step(m, "rau_backward_select", hop_w, select_w)
    m.zero_grads()
    m.forward()
    t_gt = targets(m.argmax(), batch)
    ddp = joint.bce_grad(m.dopred(), t_gt, f32(select_w))
    assert ddp.dtype == np.float32 and 0 < t_gt.sum() < t_gt.size
    dev = on_device({"dopred": ddp})
    assert raw_ext(m, hop_w, None, None, None, dev) == 0
    same_bits(m.get_grads(), base)
    m.close()


def test_no_gradients_is_rau_backward_merged_bit_for_bit_and_launch_for_launch():
    sh, batch, params, masks = problem("SMALL")
    hop_w, select_w, merge_w = [3, 3, 3], [0.7, 0, 1.3], [0.7, 1.3]
    m = make_model(sh, params, masks)
    put(m, batch)
    m.prof_enable()

    def run(call):
        m.prof_reset()
        m.zero_grads()
        m.forward()
        assert call() == 0
        g = m.get_grads()
        return g, {n: v["launches"] for n, v in m.prof().items() if v["launches"]}

    for sw, mw in ((None, None), (select_w, merge_w)):
        base, listing = run(lambda: builtin(m, "rau_backward_merged", hop_w, sw, None, mw))
        for struct in (False, True):
            got, ls = run(lambda: raw_ext(m, hop_w, sw, None, mw, None, struct=struct))
            same_bits(got, base)
            assert ls == listing and not any(n.startswith("ext_") for n in ls)
    # the Python form: an empty dict of gradients
    m.zero_grads(); m.forward(); m.backward(f32(hop_w), f32(select_w), None, f32(merge_w), out_grads={})
    same_bits(m.get_grads(), base)
    # and with gradients the three launches are there, once each
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    dev = on_device(G)
    got, ls = run(lambda: raw_ext(m, hop_w, None, None, None, dev))
    assert (ls.get("ext_dl"), ls.get("ext_signal"), ls.get("ext_da")) == (1, 1, 1) and "scale_hops" not in ls
    m.prof_enable(False)
    m.close()


def test_two_identical_calls_give_the_same_bits():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    put(m, batch)
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    first = ext_step(m, G, [3, 3, 3], f32([0.7, 0, 1.3]))
    same_bits(ext_step(m, G, [3, 3, 3], f32([0.7, 0, 1.3])), first)
    m.close()


# ------------------------------------------------------------------------------------------ 3. bf16 mode
def test_bf16_mode_against_the_emulated_oracle():
    sh, batch, params, masks = problem("SMALL")
    hop_w = [3, 3, 3]
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    m = make_model(sh, params, masks, dtype="bf16")
    put(m, batch)
    got = ext_step(m, G, hop_w)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    F = linear_F(G)
    with RT.bf16_emulation():
        emu = ext_ref.step(sh, params, batch, masks, hop_w, F=F, bf16=True)
    nudged = []
    for n in NUDGES:
        with RT.bf16_emulation(n):
            nudged.append(ext_ref.step(sh, params, batch, masks, hop_w, F=F, bf16=True))
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    err = lambda a, b: float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    bad, ratio = {}, 0.0
    for grp in GROUPS:
        for name, sl in util.layer_slices(layouts[grp]):
            r = emu["g_" + grp][sl]
            flip = max(err(x["g_" + grp][sl], r) for x in nudged)
            tol = TOL_BASE + one_flip + SAFETY * flip
            e = err(got[grp][sl], r)
            ratio = max(ratio, e / tol)
            if not e < tol:
                bad[name] = (e, tol)
    print(f"bf16 ext: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated oracle, (error, derived bar): {bad}"


# ------------------------------------------------------------------------------------------ 4. tied dropout
def test_tied_feature_map_dropout():
    sh, batch, params, masks = problem("SMALL")
    tied = dict(masks, x=np.ascontiguousarray(masks["x"][0]))                  # hop 0's mask is the tied one
    replicated = dict(masks, x=np.ascontiguousarray(np.broadcast_to(tied["x"], (sh.H,) + tied["x"].shape)))
    m = make_model(sh, params)
    m.tie_feature_dropout()
    m.set_masks(tied)
    put(m, batch)
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    got = ext_step(m, G, [3, 3, 3])
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = ext_ref.step(sh, params, batch, replicated, [3, 3, 3], F=linear_F(G))
    assert_within(got, ref, layouts, "tied")


# ------------------------------------------------------------------------------------------ 5. autograd bridge
def kd_entropy(scores, dps, atts, teacher, T=2.0):
    """Temperature-T KL of the uni row to fixed teacher logits (batch mean, times T^2) + 0.1 x the mean attention
    entropy of every hop.  do_pred is not used.  Written on torch tensors of either dtype."""
    uni = sum(scores) / len(scores)
    p = torch.softmax(teacher / T, dim=1)
    kl = (p * (torch.log_softmax(teacher / T, dim=1) - torch.log_softmax(uni / T, dim=1))).sum(1).mean() * T * T
    ent = sum(-(a * torch.log(a + 1e-12)).sum(1).mean() for a in atts)
    return kl + 0.1 * ent


def test_autograd_step_with_a_nonlinear_loss():
    from rau_vqa_amd import autograd
    sh, batch, params, masks = problem("SMALL")
    hop_w = [3, 0.5, 2]
    teacher = np.random.default_rng(9).normal(size=(sh.B, sh.K))
    m = make_model(sh, params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    put(m, batch)
    t_dev = torch.as_tensor(teacher, dtype=torch.float32).cuda()

    def total_loss():
        m.zero_grads()
        logits, dopred, attprob = autograd.step(m, hop_w=f32(hop_w))
        assert logits.requires_grad and dopred.requires_grad and attprob.requires_grad
        loss = kd_entropy(list(logits), list(dopred), list(attprob), t_dev)
        loss.backward()
        return float(loss.detach()) + float(np.dot(f32(hop_w), m.losses()))

    m.prof_enable()
    m.prof_reset()
    first = total_loss()
    got = m.get_grads()
    ls = {n: v["launches"] for n, v in m.prof().items() if v["launches"]}
    m.prof_enable(False)
    # the unused output arrived as None and went in as NULL: its launch is not there, the other two are
    assert "ext_signal" not in ls and ls.get("ext_dl") == 1 and ls.get("ext_da") == 1
    F = lambda s, d, a: kd_entropy(s, d, a, torch.as_tensor(teacher))
    ref = ext_ref.step(sh, params, batch, masks, hop_w, F=F)
    assert_within(got, ref, layouts, "autograd")
    assert abs(float(first) - (ref["ext"] + float(np.dot(hop_w, _hop_ce(ref, batch))))) < 1e-4 * abs(first)
    # a second step after an update trains on
    losses = [first]
    for it in range(3):
        m.update(it, lr=3e-3, mult_lr=3e-3, eta=0.0)
        losses.append(total_loss())
    print("loss over 3 updates:", [f"{v:.5f}" for v in losses])
    assert losses[-1] < losses[0], losses
    m.close()


def _hop_ce(ref, batch):
    lg = torch.as_tensor(ref["logits"])
    y = torch.as_tensor(batch["labels"]).long() - 1
    return np.array([float(torch.nn.functional.cross_entropy(lg[h], y)) for h in range(lg.shape[0])])


# ------------------------------------------------------------------------------------------ 6. state and errors
def test_state_and_errors():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    lib, h = m._lib, m._h
    G = seeded_G(sh.H, sh.B, sh.K, sh.S)
    dev = on_device(G)
    out = [C.c_void_p() for _ in range(3)]
    pitch = C.c_int32()
    put(m, batch)
    assert lib.rau_outputs_dev(h, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(pitch)) == STATE
    with pytest.raises(L.RauError):
        m.output_tensors()
    m.forward()
    assert lib.rau_outputs_dev(h, C.byref(out[0]), None, None, C.byref(pitch)) == 0 and pitch.value == 12
    assert lib.rau_outputs_dev(h, None, None, None, None) == 0
    # a misaligned d_logits: refused, and the forward is still there to be used
    big = torch.zeros(sh.H * sh.B * sh.K + 4, device="cuda")
    mis = L.RauOutGrads(big.data_ptr() + 4, None, None)
    hp = f32([3, 3, 3])
    m.zero_grads()
    assert lib.rau_backward_ext(h, ptr(hp), None, None, None, C.byref(mis)) == INVALID
    assert b"16-byte" in lib.rau_last_error()
    assert lib.rau_backward_ext(h, None, None, None, None, None) == INVALID     # no hop_w and no gradient
    assert raw_ext(m, [3, np.nan, 3], None, None, None, dev) == INVALID
    assert raw_ext(m, [3, 3, 3], None, None, None, dev) == 0
    first = m.get_grads()
    # one backward per forward
    assert raw_ext(m, [3, 3, 3], None, None, None, dev) == STATE
    same_bits(m.get_grads(), first)
    # built-in terms on a batch without labels: refused with the gradients untouched; external-only runs
    put(m, batch, labelled=False)
    m.forward()
    for ws in (([3, 3, 3], None, None, None), (None, [0.7, 0, 1.3], None, None), (None, None, None, [0.7, 1.3])):
        assert raw_ext(m, *ws, dev) == STATE
    same_bits(m.get_grads(), first)
    assert raw_ext(m, [0, 0, 0], [0, 0, 0], None, [0, 0], dev) == 0
    # a wrong shape in the Python form
    put(m, batch)
    m.forward()
    with pytest.raises(ValueError):
        m.backward(hp, out_grads={"logits": dev["logits"][:, :-1]})
    with pytest.raises(ValueError):
        m.backward(hp, out_grads={"logit": dev["logits"]})
    with pytest.raises(ValueError):
        m.backward(hp, out_grads={"dopred": dev["dopred"].cpu()})
    m.close()


def test_graph_step_replays_unchanged_after_an_ext_backward():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    put(m, batch)
    hp = f32([3, 3, 3])
    L.check(m._lib.rau_graph_step(m._h, ptr(hp), 1))
    before = m.get_grads()
    ext = ext_step(m, seeded_G(sh.H, sh.B, sh.K, sh.S), [3, 3, 3])
    assert any(not np.array_equal(ext[k], before[k]) for k in GROUPS)
    L.check(m._lib.rau_graph_step(m._h, ptr(hp), 1))
    same_bits(m.get_grads(), before)
    m.close()


def test_sigmoid_answer_criterion():
    from tests import bce_ref
    sh, batch, params, masks = problem("SMALL")
    hop_w = [3, 0.5, 2]
    G = pick(seeded_G(sh.H, sh.B, sh.K, sh.S), "l")
    m = make_model(sh, params, masks)
    m.set_answer_loss("bce")
    put(m, batch)
    m.forward()
    dev = on_device(G)
    assert raw_ext(m, hop_w, None, None, [0.7, 1.3], dev) == INVALID          # the merged rows stay refused
    got = ext_step(m, G, hop_w)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = ext_ref.step(sh, params, batch, masks, hop_w, F=linear_F(G), loss="bce")
    assert_within(got, ref, layouts, "bce + F")
    # ext_ref's statement of the criterion is bce_ref's: without F the two agree
    a = bce_ref.step(sh, params, batch, masks, hop_w)
    b = ext_ref.step(sh, params, batch, masks, hop_w, loss="bce")
    for k in GROUPS:
        assert util.rel_err(b["g_" + k], a["g_" + k]) < 1e-12, k
