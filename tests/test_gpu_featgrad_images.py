"""The per-image feature-map gradient on the GPU: rau_set_feat_grad(ctx, RAU_FEAT_GRAD_IMAGES) on image-table batches
(k_xgrad_accum_img in xgrad.hip, rau_set_batch_dev_images, rau_feat_grad_rows, autograd.step(feats=table)).

The oracle is tests/featgrad_ref.step, unchanged, with the TABLE as the leaf and pre = T -> T[image_of] in front of
the library: its g_feats is then the gradient at the table, [N,D,S].  The bar is TOL = 1e-4, the file's standing
gradient tolerance (tests/test_gpu_featgrad.py); bit comparisons are np.array_equal on the uint32 views.

Shapes are those of tests/test_gpu_featgrad.py: SMALL (S = 12), SMALL_S49 (pitch 52: the mask indexed over the logical
tensor), X196 (D = 136 = 8.5 row blocks of 16, S = 196: 16-byte accesses over 49 quads per row, regenerated bits) and
X196_B5 (a batch remainder).  The table: image_of = [2, 0, 2, 2, 0, 3] cut to the batch size (repeated cyclically
where the batch is larger: SMALL has 8 samples, the bf16 shape 12) with N = 4 -- non-monotone, a fan-out of three or
more, image 1 named by nobody.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from rau_vqa_amd import feat16
from rau_vqa_amd.model import regions_of
from tests import ext_ref, featgrad_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_featgrad import HOP_W, X196, assert_dx, launches, on_device, problem, seeded_G
from tests.test_gpu_packed import pack
from tests.test_gpu_select import GROUPS, INVALID, STATE, TOL, f32, grad_errs, make_model, same_bits

pytestmark = pytest.mark.gpu

N_IMG = 4
BASE = [2, 0, 2, 2, 0, 3]


def table_of(sh, batch, n_images=N_IMG, base=BASE, first=0):
    """(table [N,D,S], image_of [B]) cut from the problem's own maps."""
    image_of = np.resize(np.array(base, np.int32), sh.B)
    return np.ascontiguousarray(batch["feats"][first:first + n_images]), image_of


def put_table(m, batch, table, image_of, labelled=True, **kw):
    m.set_batch(table, batch["tokens"], batch["lens"], batch["labels"] if labelled else None, image_of=image_of, **kw)


def run(m, hop_w, out_grads=None, graph=False):
    """One step on the resident batch -> the parameter gradients."""
    if graph:
        m.graph_step(f32(hop_w))
    else:
        m.zero_grads()
        m.forward()
        m.backward(None if hop_w is None else f32(hop_w), out_grads=out_grads)
    return m.get_grads()


def step(m, hop_w, out_grads=None, graph=False):
    grads = run(m, hop_w, out_grads, graph)
    return m.feature_grad(), grads


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def unnamed(image_of, n_images):
    return sorted(set(range(n_images)) - set(int(i) for i in image_of))


def image_counts(sh):
    """Region counts per IMAGE: a full map, a single position and two between."""
    return np.minimum(np.array([sh.S, 7, 1, 5], np.int32), sh.S).astype(np.int32)


# ------------------------------------------------------------------------------------------ 1. oracle parity
VARIANTS = ("explicit", "philox", "evaluate", "tied", "regions", "trailing_zero", "ext_only", "bce")
CASES = [(n, v) for n in ("SMALL_S49", "X196") for v in VARIANTS] + [("SMALL", "explicit"), ("X196_B5", "explicit"),
                                                                     ("X196_B5", "philox")]


@pytest.mark.parametrize("name,variant", CASES)
def test_against_the_oracle(name, variant):
    sh, batch, params, masks = problem(name)
    table, image_of = table_of(sh, batch)
    hop_w, ref_kw, put_kw, out_grads, labelled = HOP_W, {}, {}, None, True
    ref_masks = masks
    m = make_model(sh, params, None if variant in ("philox", "evaluate", "tied") else masks)
    if variant == "philox":
        m.set_dropout_seed(7, 3)
        ref_masks = {k: m.get_mask(k) for k in masks}
    elif variant == "evaluate":
        m.evaluate()
        ref_masks = None
    elif variant == "tied":
        m.tie_feature_dropout()
        tied = dict(masks, x=np.ascontiguousarray(masks["x"][0]))
        m.set_masks(tied)
        ref_masks = dict(masks, x=np.ascontiguousarray(np.broadcast_to(tied["x"], (sh.H,) + tied["x"].shape)))
    elif variant == "regions":
        put_kw["regions"] = image_counts(sh)                       # per image: set_batch gathers them (regions_of)
        ref_kw["nreg"] = regions_of(image_counts(sh), image_of)
    elif variant == "trailing_zero":
        hop_w = [3, 2, 0]
    elif variant == "ext_only":
        G = seeded_G(sh.H, sh.B, sh.K, sh.S)
        out_grads, hop_w, labelled = on_device(G), None, False
        ref_kw["F"] = ext_ref.linear_F(G["logits"], G["dopred"], G["attprob"])
    elif variant == "bce":
        m.set_answer_loss("bce")
        ref_kw["loss"] = "bce"
    # the same batch with the switch off.  (Evaluate mode: its table forward has no backward with the switch off,
    # so there the plain batch table[image_of], whose results are the table batch's bit for bit.)
    if variant == "evaluate":
        m.set_batch(np.ascontiguousarray(table[image_of]), batch["tokens"], batch["lens"], batch["labels"])
    else:
        put_table(m, batch, table, image_of, labelled, **put_kw)
    off = run(m, hop_w, out_grads)
    m.want_feature_grad(per_image=True)
    assert m.feature_grad_wanted and m.feature_grad_mode == L.FEAT_GRAD_IMAGES == 2
    put_table(m, batch, table, image_of, labelled, **put_kw)
    m.prof_enable()
    dT, on = step(m, hop_w, out_grads)
    ls = launches(m)
    rows = m.feature_grad_rows()
    m.close()
    assert rows == N_IMG and dT.shape == (N_IMG, sh.D, sh.S)
    # the per-image pass behind every hop's product; the per-sample pass and the fused kernel never run
    assert "xgrad_accum" not in ls and ls.get("xgrad_accum_img", 0) >= 1, ls
    assert ls["xgrad_accum_img"] == ls.get("conv_embed_dgrad"), ls
    same_bits(on, off)
    idx = torch.as_tensor(image_of).long()
    ref = featgrad_ref.step(sh, params, dict(batch, feats=table, labels=batch["labels"] if labelled else None),
                            ref_masks, hop_w, pre=lambda T: T[idx], **ref_kw)
    assert ref["g_feats"].shape == dT.shape
    assert_dx(dT, ref["g_feats"], f"{name} {variant} per image")
    none = unnamed(image_of, N_IMG)
    assert 1 in none
    for i in range(N_IMG):
        assert dT[i].any() == (i not in none), i                  # exact zeros for an image nobody names
    if variant == "regions":
        n = image_counts(sh)
        for i in range(N_IMG):
            assert not dT[i, :, n[i]:].any(), i                   # exactly zero behind each image's count


# ------------------------------------------------------------------------------------------ 2. identity table
@pytest.mark.parametrize("name,variant", [(n, v) for n in ("X196", "SMALL_S49") for v in ("explicit", "philox", "evaluate")])
def test_identity_table_has_the_bits_of_the_plain_batch_under_mode_1(name, variant):
    sh, batch, params, masks = problem(name)
    m = make_model(sh, params, masks if variant == "explicit" else None)
    if variant == "philox":
        m.set_dropout_seed(7, 3)
    elif variant == "evaluate":
        m.evaluate()
    m.want_feature_grad()
    assert m.feature_grad_mode == L.FEAT_GRAD_SAMPLES
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    dX, plain = step(m, HOP_W)
    m.want_feature_grad(per_image=True)
    put_table(m, batch, batch["feats"], np.arange(sh.B, dtype=np.int32))
    dT, table = step(m, HOP_W)
    m.close()
    assert dX.any() and bits_equal(dT, dX)
    same_bits(table, plain)


# ------------------------------------------------------------------------------------------ 3. plain batch, mode 2
@pytest.mark.parametrize("name", ["X196", "SMALL_S49"])
def test_a_plain_batch_under_mode_2_is_mode_1(name):
    sh, batch, params, masks = problem(name)
    m = make_model(sh, params, masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.prof_enable()
    res = {}
    for per_image in (False, True):
        m.want_feature_grad(per_image=per_image)
        m.prof_reset()
        dX, grads = step(m, HOP_W)
        res[per_image] = (dX, grads, launches(m), m.feature_grad_rows())
    m.close()
    assert res[True][2] == res[False][2] and "xgrad_accum_img" not in res[True][2], res[True][2]
    assert res[True][3] == res[False][3] == sh.B
    assert bits_equal(res[True][0], res[False][0])
    same_bits(res[True][1], res[False][1])


# ------------------------------------------------------------------------------------------ 4. determinism and capture
@pytest.mark.parametrize("name,variant", [("X196", "philox"), ("X196", "explicit"), ("SMALL_S49", "explicit")])
def test_repeated_and_captured_steps_give_the_eager_bits_for_any_table(name, variant):
    """The captured launches carry neither N nor the sample lists: a replay on a later table batch with another N
    and another image_of is that batch's eager step."""
    sh, batch, params, masks = problem(name)
    m = make_model(sh, params, masks if variant == "explicit" else None)
    if variant == "philox":
        m.set_dropout_seed(7, 3)
    m.want_feature_grad(per_image=True)
    table, image_of = table_of(sh, batch)
    put_table(m, batch, table, image_of)
    a, ga = step(m, HOP_W)
    b, gb = step(m, HOP_W)
    c, gc = step(m, HOP_W, graph=True)                              # the capture
    d, _ = step(m, HOP_W, graph=True)                               # a replay
    assert a.any() and bits_equal(a, b) and bits_equal(a, c) and bits_equal(a, d)
    same_bits(ga, gb)
    table2, image_of2 = table_of(sh, batch, n_images=3, base=[1, 2, 0, 0, 1, 1, 2], first=2)
    assert sorted(set(image_of2.tolist())) == [0, 1, 2]
    put_table(m, batch, table2, image_of2)
    e, ge = step(m, HOP_W, graph=True)                              # a replay on another table
    f, gf = step(m, HOP_W)
    m.close()
    assert e.shape == (3, sh.D, sh.S) and e.any() and bits_equal(e, f)
    same_bits(ge, gf)
    assert not np.array_equal(e, a[:3])


# ------------------------------------------------------------------------------------------ 5. upload paths
@pytest.mark.parametrize("name", ["X196", "SMALL_S49"])
def test_every_upload_path_gives_the_bits_of_the_synchronous_f32_table(name):
    sh, batch, params, masks = problem(name)
    table, image_of = table_of(sh, batch)
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    m = make_model(sh, params, masks)
    m.want_feature_grad(per_image=True)
    put_table(m, batch, table, image_of)
    want, gwant = step(m, HOP_W)
    # the device table: no byte of the maps crosses the bus
    x = torch.as_tensor(table).cuda()
    torch.cuda.synchronize()
    m.set_batch_dev(x, *tok, image_of=image_of)
    assert m.batch_images() == N_IMG
    got, g = step(m, HOP_W)
    assert bits_equal(got, want)
    same_bits(g, gwant)
    # an fp16 table against the f32 table of the widened values
    half = table.astype(np.float16)
    wide = feat16.widen(half, "f16")
    assert not np.array_equal(wide, table)
    put_table(m, batch, wide, image_of)
    want16, gwant16 = step(m, HOP_W)
    m.set_batch(half, *tok, feat_type="f16", image_of=image_of)
    got, g = step(m, HOP_W)
    assert bits_equal(got, want16) and not np.array_equal(want16, want)
    same_bits(g, gwant16)
    # a packed table: the counts become per-image region counts
    n_img = np.minimum(np.array([sh.S, 7, 3, 5], np.int32), sh.S).astype(np.int32)
    rows = pack(table, n_img)
    put_table(m, batch, feat16.unpack_regions(rows, n_img, sh.S), image_of, regions=n_img)
    wantp, gwantp = step(m, HOP_W)
    m.set_batch_packed(rows, n_img, *tok, image_of=image_of)
    got, g = step(m, HOP_W)
    assert bits_equal(got, wantp)
    same_bits(g, gwantp)
    # the asynchronous path: slot 1, made current by use_batch (last: the context stays on that slot)
    m.set_batch_async(1, table, *tok, image_of=image_of)
    m.use_batch(1)
    got, g = step(m, HOP_W)
    m.close()
    assert bits_equal(got, want)
    same_bits(g, gwant)


# ------------------------------------------------------------------------------------------ 6. bf16 mode
def test_bf16_mode_against_the_emulated_oracle():
    """The bar is test_gpu_featgrad.test_bf16_mode_against_the_emulated_oracle's derivation, restated: TOL_BASE + one
    flipped rounding over the shortest reduction + SAFETY x the largest shift of the nudged emulations."""
    sh = util.shapes(dict(X196, D=256, M=256, B=12))
    batch, params, masks = util.make_problem(sh, scale=0.3)
    table, image_of = table_of(sh, batch)
    m = make_model(sh, params, masks, dtype="bf16")
    m.want_feature_grad(per_image=True)
    put_table(m, batch, table, image_of)
    m.prof_enable()
    dT, _ = step(m, HOP_W)
    ls = launches(m)
    m.close()
    assert ls.get("xgrad_accum_img") == sh.H == ls.get("conv_embed_dgrad") and "xgrad_accum" not in ls, ls
    idx = torch.as_tensor(image_of).long()
    ref = lambda: featgrad_ref.step(sh, params, dict(batch, feats=table), masks, HOP_W, bf16=True,
                                    pre=lambda T: T[idx])["g_feats"]
    with RT.bf16_emulation():
        emu = ref()
    flip = 0.0
    for nudge in NUDGES:
        with RT.bf16_emulation(nudge):
            flip = max(flip, util.rel_err(ref(), emu))
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    tol = TOL_BASE + one_flip + SAFETY * flip
    print(f"bf16 per image: derived bar {tol:.2e} (nudged shift {flip:.2e})")
    assert_dx(dT, emu, "bf16 per image", tol)
    assert not dT[1].any()


# ------------------------------------------------------------------------------------------ 7. refusals and state
def test_modes_refusals_and_rows():
    sh, batch, params, masks = problem("SMALL")
    table, image_of = table_of(sh, batch)
    m = make_model(sh, params, masks)
    lib, h = m._lib, m._h
    hp = f32(HOP_W)
    rows = C.c_int32(-1)
    for bad in (3, -1, 7):
        assert lib.rau_set_feat_grad(h, bad) == INVALID and b"rau_set_feat_grad" in lib.rau_last_error()
    assert m.feature_grad_mode == L.FEAT_GRAD_OFF
    assert lib.rau_feat_grad_rows(h, C.byref(rows)) == STATE and b"rau_set_feat_grad" in lib.rau_last_error()
    # mode 1 on a table: refused, as before
    m.want_feature_grad()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    _, before = step(m, HOP_W)
    assert m.feature_grad_rows() == sh.B
    put_table(m, batch, table, image_of)
    m.forward()
    assert lib.rau_feat_grad_rows(h, C.byref(rows)) == STATE            # no backward since the forward
    assert lib.rau_backward(h, hp.ctypes.data) == STATE and b"image" in lib.rau_last_error()
    assert lib.rau_graph_step(h, hp.ctypes.data, 0) == STATE
    same_bits(m.get_grads(), before)
    # mode 2: the table's N, under rau_feat_grad_dev's state rules
    m.want_feature_grad(per_image=True)
    assert lib.rau_feat_grad_rows(h, C.byref(rows)) == STATE
    m.forward()
    assert lib.rau_feat_grad_rows(h, C.byref(rows)) == STATE
    assert lib.rau_backward(h, hp.ctypes.data) == 0
    assert lib.rau_feat_grad_rows(h, C.byref(rows)) == 0 and rows.value == N_IMG
    assert lib.rau_feat_grad_dev(h, None, None) == 0
    t = m.feature_grad_tensor()
    torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(m.stream()))
    assert tuple(t.shape) == (N_IMG, sh.D, sh.S) and np.array_equal(t.cpu().numpy(), m.feature_grad())
    m.forward()
    assert lib.rau_feat_grad_rows(h, C.byref(rows)) == STATE            # ... until the next forward
    m.close()


@pytest.mark.parametrize("per_image", [False, True])
def test_bank_batches_stay_refused_with_no_gradient_changed(per_image):
    sh, batch, params, masks = problem("SMALL")
    table, image_of = table_of(sh, batch)
    m = make_model(sh, params, masks)
    m.want_feature_grad(per_image=per_image)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    _, before = step(m, HOP_W)
    m.bank_create(sh.B)
    m.bank_put(0, table)
    m.set_batch(None, batch["tokens"], batch["lens"], batch["labels"], image_of=image_of,
                bank_rows=np.arange(N_IMG, dtype=np.int32))
    m.forward()
    hp = f32(HOP_W)
    assert m._lib.rau_backward(m._h, hp.ctypes.data) == STATE and b"bank" in m._lib.rau_last_error()
    assert m._lib.rau_graph_step(m._h, hp.ctypes.data, 0) == STATE
    same_bits(m.get_grads(), before)
    m.want_feature_grad(False)
    m.forward()
    assert m._lib.rau_backward(m._h, hp.ctypes.data) == 0
    m.close()


def test_smaller_batch_gives_the_bits_of_a_context_created_at_n():
    sh, batch, params, masks = problem("X196")
    n = 4
    shn = dataclasses.replace(sh, B=n)
    table, image_of = table_of(sh, batch)
    bn = {"tokens": np.ascontiguousarray(batch["tokens"][:, :n]), "lens": batch["lens"][:n],
          "labels": batch["labels"][:n]}
    mn = {k: np.ascontiguousarray(v[:, :n]) for k, v in masks.items()}
    m = make_model(sh, params, masks)
    m.want_feature_grad(per_image=True)
    put_table(m, batch, table, image_of)
    step(m, HOP_W)                          # the buffer and the lists are in use at the capacity first
    m.set_batch_size(n)
    assert m.feature_grad_mode == L.FEAT_GRAD_IMAGES
    with pytest.raises(L.RauError):
        m.feature_grad_rows()
    m.set_masks(mn)
    put_table(m, bn, table, image_of[:n])
    a, ga = step(m, HOP_W)
    m.close()
    fresh = make_model(shn, params, mn)
    fresh.want_feature_grad(per_image=True)
    put_table(fresh, bn, table, image_of[:n])
    b, gb = step(fresh, HOP_W)
    fresh.close()
    assert a.shape == (N_IMG, sh.D, sh.S) and a.any() and bits_equal(a, b)
    assert not a[1].any() and not a[3].any()            # [2, 0, 2, 2] names images 0 and 2 only
    same_bits(ga, gb)


# ------------------------------------------------------------------------------------------ 8. autograd.step(feats=table)
@pytest.mark.parametrize("name", ["X196", "SMALL_S49"])
def test_autograd_step_trains_a_linear_in_front_of_the_table(name):
    """A torch Linear over the channels makes the table; its gradient comes back per image from the library."""
    from rau_vqa_amd import autograd
    sh, batch, params, masks = problem(name)
    raw_np, image_of = table_of(sh, batch)
    rng = np.random.default_rng(21)
    W0 = (np.eye(sh.D) + 0.1 * rng.normal(size=(sh.D, sh.D))).astype(np.float32)
    teacher = rng.normal(size=(sh.B, sh.K)).astype(np.float32)

    def my_loss(scores, dps, atts, tch):
        uni = sum(scores) / len(scores)
        kl = -(torch.softmax(tch, 1) * torch.log_softmax(uni, 1)).sum(1).mean()
        return kl + 0.1 * sum(-(a * torch.log(a + 1e-12)).sum(1).mean() for a in atts) + 0.05 * sum(d.mean() for d in dps)

    m = make_model(sh, params, masks)
    m.want_feature_grad(per_image=True)
    lin = torch.nn.Linear(sh.D, sh.D, bias=False).cuda()
    with torch.no_grad():
        lin.weight.copy_(torch.as_tensor(W0))
    own = torch.cuda.ExternalStream(m.stream())

    def one_run():
        lin.weight.grad = None
        raw = torch.as_tensor(raw_np).cuda().requires_grad_(True)
        x = lin(raw.transpose(1, 2)).transpose(1, 2).contiguous()          # the table [N, D, S]
        x.retain_grad()
        own.wait_stream(torch.cuda.current_stream())
        m.set_batch_dev(x.detach(), batch["tokens"], batch["lens"], batch["labels"], image_of=image_of)
        m.zero_grads()
        logits, dopred, attprob = autograd.step(m, hop_w=f32(HOP_W), feats=x)
        my_loss(list(logits), list(dopred), list(attprob), torch.as_tensor(teacher).cuda()).backward()
        return x.grad.cpu().numpy(), lin.weight.grad.cpu().numpy(), m.get_grads()

    got_x, got_w, got_p = one_run()
    again_x, _, again_p = one_run()
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    assert got_x.shape == (N_IMG, sh.D, sh.S) and bits_equal(got_x, again_x)
    same_bits(got_p, again_p)

    idx = torch.as_tensor(image_of).long()
    Wt = torch.as_tensor(W0, dtype=torch.float64).requires_grad_(True)
    F = lambda s, d, a: my_loss(s, d, a, torch.as_tensor(teacher, dtype=torch.float64))
    ref = featgrad_ref.step(sh, params, dict(batch, feats=raw_np), masks, HOP_W, F=F,
                            pre=lambda f: torch.einsum("ed,nds->nes", Wt, f)[idx], pre_params=(Wt,))
    # the gradient at the table itself: the same restatement with the stage's OUTPUT as the leaf
    x_np = np.einsum("ed,nds->nes", W0.astype(np.float64), raw_np.astype(np.float64))
    ref_x = featgrad_ref.step(sh, params, dict(batch, feats=x_np), masks, HOP_W, F=F, pre=lambda T: T[idx])
    assert_dx(got_x, ref_x["g_feats"], f"{name} table.grad")
    assert_dx(got_w, ref["g_pre"][0], f"{name} Linear weight gradient")
    assert not got_x[1].any()
    errs = grad_errs(got_p, ref, layouts)
    assert all(v < TOL for v in errs.values()), {k: v for k, v in errs.items() if not v < TOL}
