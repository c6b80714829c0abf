"""Per-position L2 normalisation of the feature maps on the GPU (rau_set_feat_norm, featnorm.hip, rau_dev_l2norm).

What fixes the bits.  The normalised maps xn are compared with the float64 statement under a DERIVED bound (test 1);
everything behind them is tied to the library itself: a context with the switch on gives, bit for bit, what a context
with the switch off gives for xn as a plain float32 batch (test 2), and every batch form gives the plain batch's bits
(test 3).  The fp64 oracle on float64-normalised maps (tests/featnorm_ref.py) closes the loop at the project's bar
of 1e-4 (tests 4 and 5).

The bound of test 1.  A sum of D rounded squares in any fixed order has relative error at most (D + 1) 2^-24; the
square root halves that; the 1-ulp hardware square root, the division and the product add theirs: every element with
|reference| > 2^-100 is within (D/2 + 4) 2^-24 relative, every norm within (D/2 + 2) 2^-24.

Shapes: B = 3, H = 2, T = 4, the smallest legal widths (4), K = 8.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from rau_vqa_amd import _lib as L
from rau_vqa_amd import feat16
from tests import featnorm_ref, util
from tests.test_gpu_select import GROUPS, INVALID, STATE, TOL, f32, grad_errs, make_model, same_bits

pytestmark = pytest.mark.gpu

EPS = 1e-3
HOP_W = [2.0, 0.5]
U = 2.0 ** -24
NUM_SHAPES = [(4, 5), (36, 49), (512, 196), (2048, 16), (36, 900)]     # 900: the fused attention family's bound
TYPES = ("f32", "f16", "bf16", "e4m3", "e5m2")
_CACHE = {}


def dims(D, S, **over):
    d = dict(B=3, T=4, V=20, E=4, Rq=4, D=D, S=S, M=4, A=4, R=4, K=8, H=2)
    d.update(over)
    return d


def problem(D, S, **over):
    key = (D, S, tuple(sorted(over.items())))
    if key not in _CACHE:
        sh = util.shapes(dims(D, S, **over))
        _CACHE[key] = (sh,) + util.make_problem(sh, scale=0.5)
    sh, batch, params, masks = _CACHE[key]
    return sh, dict(batch), params, masks


def special_maps(n, D, S, seed=3):
    """[n, D, S] float32: position 1 of map 0 all zero, position 2 of map 1 of norm 1e-5 (< EPS), every other norm
    at least 2 EPS."""
    x = np.random.default_rng(seed).normal(size=(n, D, S)).astype(np.float32)
    x[0, :, 1] = 0.0
    col = x[1, :, 2].astype(np.float64)
    x[1, :, 2] = (col * (1e-5 / np.sqrt(np.sum(col * col)))).astype(np.float32)
    nrm = np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=1))
    nrm[0, 1] = nrm[1, 2] = 1.0
    assert nrm.min() >= 2 * EPS
    return x


def as_type(x, ft):
    out = np.empty(x.shape, feat16.dtype_of(ft))
    feat16.store(out, x, ft)
    return out


def cuda(a):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def host(m, t):
    m.sync()
    return t.cpu().numpy()


def check_numbers(xn, nrm, x, D, what):
    """xn [n,D,S], nrm [n,S] (float32) against the float64 statement of the float32 maps x, under the derived bound."""
    ref, ref_n = featnorm_ref.normalize64(x, EPS)
    big = np.abs(ref) > 2.0 ** -100
    err = np.max(np.abs(xn.astype(np.float64) - ref)[big] / np.abs(ref)[big])
    live = ref_n > 0
    err_n = np.max(np.abs(nrm.astype(np.float64) - ref_n)[live] / ref_n[live])
    print(f"{what}: xn rel err {err / U:.2f} ulp (bound {D / 2 + 4}), nrm {err_n / U:.2f} ulp (bound {D / 2 + 2})")
    assert err <= (D / 2 + 4) * U and err_n <= (D / 2 + 2) * U
    assert np.all(xn[~big] == 0)
    # the all-zero position: exact +0, norm 0
    assert np.all(xn[0, :, 1] == 0) and not np.any(np.signbit(xn[0, :, 1])) and nrm[0, 1] == 0
    assert not np.signbit(nrm[0, 1])


def pitched(m):
    """The pitched device buffers behind rau_norm_feats_dev as numpy: xn [rows, D, pitch], nrm [rows, pitch]."""
    from rau_vqa_amd.dist import device_view
    xn, nrm, pitch, rows = m._norm_feats_dev()
    D, dev = m.cfg.D, m.cfg.device_id
    return (host(m, device_view(xn, rows * D * pitch, dev).view(rows, D, pitch)),
            host(m, device_view(nrm, rows * pitch, dev).view(rows, pitch)))


def put(m, batch, feats=None, **kw):
    m.set_batch(batch["feats"] if feats is None else feats, batch["tokens"], batch["lens"], batch["labels"], **kw)


def run_step(m, graph=False, seed=(7, 3)):
    """zero_grads + forward + backward under the seeded masks; every output and the three gradient groups."""
    m.set_dropout_seed(*seed)
    if graph:
        m.graph_step(f32(HOP_W))
    else:
        m.zero_grads()
        m.forward()
        m.backward(f32(HOP_W))
    out = {"logits": m.logits(), "losses": m.losses(), "dopred": m.dopred(), "att": m.attention()}
    out.update(m.get_grads())
    return out


def forward_only(m):
    m.forward()
    return {"logits": m.logits(), "losses": m.losses(), "dopred": m.dopred(), "att": m.attention()}


def assert_same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


# ------------------------------------------------------------------------------------------ 1. the numbers
@pytest.mark.parametrize("D,S", NUM_SHAPES)
def test_numbers_against_the_float64_statement(D, S):
    sh, batch, params, _ = problem(D, S)
    x = special_maps(3, D, S)
    m = make_model(sh, params)
    xd = cuda(x)
    y, nrm = m.l2norm(xd, eps=EPS)
    y, nrm = host(m, y), host(m, nrm)
    check_numbers(y, nrm, x, D, f"rau_dev_l2norm D={D} S={S}")
    # in place, and again: the same bits
    y2, nrm2 = m.l2norm(xd, eps=EPS, out=xd)
    assert y2.data_ptr() == xd.data_ptr()
    assert np.array_equal(host(m, y2).view(np.uint32), y.view(np.uint32))
    assert np.array_equal(host(m, nrm2).view(np.uint32), nrm.view(np.uint32))
    # the step path's pass over the pitched batch: the same bound, and +0 in the pad columns of both buffers
    m.normalize_features(eps=EPS)
    m.evaluate()
    put(m, batch, feats=x)
    m.forward()
    xn, nr = m.norm_feats()
    check_numbers(xn, nr, x, D, f"step path D={D} S={S}")
    xp, nrp = pitched(m)
    pitch = xp.shape[2]
    assert pitch == (S + 3) // 4 * 4 and xp.shape[0] == 3
    assert np.array_equal(xp[:, :, :S].view(np.uint32), xn.view(np.uint32))
    assert np.array_equal(nrp[:, :S].view(np.uint32), nr.view(np.uint32))
    if pitch > S:
        assert not np.any(xp[:, :, S:].view(np.uint32)) and not np.any(nrp[:, S:].view(np.uint32))
    tx, tn = m.norm_feats_tensors()
    assert np.array_equal(host(m, tx), xn) and np.array_equal(host(m, tn), nr)
    m.close()


# ------------------------------------------------------------------------------------------ 2. plumbing, bit for bit
@pytest.mark.parametrize("mode", ["train", "evaluate", "tied", "bf16"])
def test_switch_on_is_switch_off_on_the_normalised_maps(mode):
    sh, batch, params, _ = problem(8, 49)
    dtype = "bf16" if mode == "bf16" else "f32"
    on, off = make_model(sh, params, dtype=dtype), make_model(sh, params, dtype=dtype)
    on.normalize_features(eps=EPS)
    assert on.features_normalized == (L.XNORM_L2, pytest.approx(EPS)) and off.features_normalized[0] == L.XNORM_NONE
    for m in (on, off):
        if mode == "evaluate":
            m.evaluate()
        if mode == "tied":
            m.tie_feature_dropout()
    x = special_maps(3, 8, 49, seed=11) * np.float32(4.0)
    for ft in TYPES:
        stored = as_type(x, ft)
        put(on, batch, feats=stored, feat_type=ft)
        a = run_step(on)
        xn, _ = on.norm_feats()
        # xn is the normalisation of the WIDENED stored values
        check = feat16.l2_normalize(feat16.widen(stored, ft), EPS)
        assert np.max(np.abs(xn - check)) <= (8 / 2 + 4) * U * np.max(np.abs(check)), ft
        put(off, batch, feats=xn)
        b = run_step(off)
        assert_same(a, b, (mode, ft))
    on.close()
    off.close()


# ------------------------------------------------------------------------------------------ 3. every batch form
def fp8_table(N, D, S, seed=5):
    """An image table whose values e4m3 holds exactly (so a bank of that type stores these very maps)."""
    raw = np.random.default_rng(seed).normal(size=(N, D, S)).astype(np.float32) * np.float32(3.0)
    return feat16.widen(as_type(raw, "e4m3"), "e4m3").astype(np.float32)


@pytest.mark.parametrize("mode", ["train", "evaluate"])
def test_every_batch_form_gives_the_plain_batch(mode):
    sh, batch, params, _ = problem(8, 49)
    image_of = np.array([1, 0, 1], np.int32)
    table = fp8_table(2, 8, 49)
    plain = np.ascontiguousarray(table[image_of])
    m = make_model(sh, params)
    m.normalize_features(eps=EPS)
    if mode == "evaluate":
        m.evaluate()
    step = (lambda: run_step(m)) if mode == "train" else (lambda: forward_only(m))
    put(m, batch, feats=plain)
    ref = step()
    ref_xn, ref_nrm = m.norm_feats()
    assert ref_xn.shape[0] == 3

    def check(what, rows=3):
        got = step()
        assert_same(got, ref, (mode, what))
        xn, nrm = m.norm_feats()
        assert xn.shape[0] == rows, what
        pick = image_of if rows == 2 else np.arange(3)
        # a map gives the same bits as a table row and as a sample's map
        assert np.array_equal(xn[pick].view(np.uint32), ref_xn.view(np.uint32)), what
        assert np.array_equal(nrm[pick].view(np.uint32), ref_nrm.view(np.uint32)), what

    n_table = 2 if mode == "evaluate" else 3   # the evaluate-mode table forward normalises the N table rows
    put(m, batch, feats=table, image_of=image_of)
    check("image table", n_table)
    m.bank_create(4, "e4m3")
    m.bank_put(1, table)
    m.set_batch(None, batch["tokens"], batch["lens"], batch["labels"], bank_rows=np.array([1, 2], np.int32),
                image_of=image_of)
    check("e4m3 bank", n_table)
    plain_dev = cuda(plain)     # (alive until the copy has run)
    m.set_batch_dev(plain_dev, batch["tokens"], batch["lens"], batch["labels"])
    check("set_batch_dev")
    m.set_batch_async(1, plain, batch["tokens"], batch["lens"], batch["labels"])
    m.use_batch(1)
    check("asynchronous slot")
    m.set_batch_async(0, table, batch["tokens"], batch["lens"], batch["labels"], image_of=image_of)
    m.use_batch(0)
    check("asynchronous slot, table", n_table)
    # packed rows bring region counts: their plain batch is the unpacked maps with the same counts
    counts = np.array([49, 7, 30], np.int32)
    rows = np.concatenate([plain[b, :, :counts[b]].T for b in range(3)]).astype(np.float32)
    put(m, batch, feats=feat16.unpack_regions(rows, counts, 49), regions=counts)
    ref = step()
    ref_xn, ref_nrm = m.norm_feats()
    m.set_batch_packed(rows, counts, batch["tokens"], batch["lens"], batch["labels"])
    check("packed rows")
    m.close()


# ------------------------------------------------------------------------------------------ 4. the fp64 oracle
@pytest.mark.parametrize("S", [49, 196, 900])
def test_against_the_oracle_on_float64_normalised_maps(S):
    sh, batch, params, masks = problem(8, S)
    batch["feats"] = special_maps(3, 8, S, seed=13)
    ref = featnorm_ref.step(sh, params, batch, masks, f32(HOP_W), EPS)
    m = make_model(sh, params, masks)
    m.normalize_features(eps=EPS)
    put(m, batch)
    m.zero_grads()
    m.forward()
    m.backward(f32(HOP_W))
    out, grads = m.outputs(), m.get_grads()
    errs = {k: util.rel_err(out[k], ref[k]) for k in ("logits", "losses", "dopred", "att")}
    errs.update(grad_errs(grads, ref, {k: m.layout(k) for k in GROUPS}))
    m.close()
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), {k: v for k, v in errs.items() if v >= TOL}


# ------------------------------------------------------------------------------------------ 5. feature-map gradient
def assert_maps(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for i in range(ref.shape[0]):
        e = util.rel_err(got[i], ref[i])
        at = np.unravel_index(np.argmax(np.abs(got[i] - ref[i])), ref[i].shape)
        print(f"{what}: map {i} rel_err {e:.2e} at {tuple(int(k) for k in at)} (max |dX| {np.max(np.abs(ref[i])):.2e})")
        assert e < TOL, (what, i, e)


@pytest.mark.parametrize("per_image", [False, True])
def test_feature_gradient_through_the_normalisation(per_image):
    sh, batch, params, masks = problem(8, 49)
    image_of = np.array([1, 0, 1], np.int32) if per_image else None      # three questions on two images
    maps = special_maps(2 if per_image else 3, 8, 49, seed=17)
    batch["feats"] = maps
    ref = featnorm_ref.feat_step(sh, params, batch, masks, f32(HOP_W), EPS, image_of=image_of)
    assert np.max(np.abs(ref["g_feats"][1, :, 2])) > 0      # the position under eps has a gradient: G / eps
    m = make_model(sh, params, masks)
    m.normalize_features(eps=EPS)
    m.want_feature_grad(per_image=per_image)

    def once():
        put(m, batch, image_of=image_of)
        m.zero_grads()
        m.forward()
        m.backward(f32(HOP_W))
        return m.feature_grad(), m.get_grads()
    dX, grads = once()
    assert m.feature_grad_rows() == maps.shape[0]
    assert_maps(dX, ref["g_feats"], "per image" if per_image else "per sample")
    errs = grad_errs(grads, ref, {k: m.layout(k) for k in GROUPS})
    assert all(v < TOL for v in errs.values()), errs
    dX2, grads2 = once()
    assert np.array_equal(dX.view(np.uint32), dX2.view(np.uint32))
    same_bits(grads, grads2)
    m.close()


def test_an_unnamed_image_keeps_its_zero_row():
    sh, batch, params, masks = problem(8, 49)
    batch["feats"] = special_maps(3, 8, 49, seed=19)
    m = make_model(sh, params, masks)
    m.normalize_features(eps=EPS)
    m.want_feature_grad(per_image=True)
    put(m, batch, image_of=np.array([2, 0, 2], np.int32))
    m.zero_grads()
    m.forward()
    m.backward(f32(HOP_W))
    dX = m.feature_grad()
    assert dX.shape[0] == 3 and not np.any(dX[1].view(np.uint32)) and np.any(dX[0]) and np.any(dX[2])
    m.close()


@pytest.mark.parametrize("D,S", NUM_SHAPES)
def test_dev_backward_against_float64_autograd(D, S):
    sh, _, params, _ = problem(D, S)
    x = special_maps(3, D, S)
    g = np.random.default_rng(23).normal(size=x.shape).astype(np.float32)
    ref = featnorm_ref.normalize_grad64(x, g, EPS)
    m = make_model(sh, params)
    xd, gd = cuda(x), cuda(g)      # (alive until the launches that read them have run: the calls do not synchronise)
    y, nrm = m.l2norm(xd, eps=EPS)
    dx = host(m, m.l2norm_backward(y, nrm, gd, eps=EPS))
    assert_maps(dx, ref, f"rau_dev_l2norm_backward D={D} S={S}")
    assert util.rel_err(dx, feat16.l2_normalize_grad(x, g, EPS)) < TOL      # the numpy statement says the same
    # in place on g, and the same bits
    dx2 = m.l2norm_backward(y, nrm, gd, eps=EPS, out=gd)
    assert dx2.data_ptr() == gd.data_ptr() and np.array_equal(host(m, dx2).view(np.uint32), dx.view(np.uint32))
    m.close()


def test_autograd_step_hands_torch_the_gradient_at_the_raw_maps():
    from rau_vqa_amd import autograd
    sh, batch, params, masks = problem(8, 49)
    m = make_model(sh, params, masks)
    m.normalize_features(eps=EPS)
    m.want_feature_grad()
    x = cuda(special_maps(3, 8, 49, seed=29)).requires_grad_(True)
    own = torch.cuda.ExternalStream(m.stream())
    own.wait_stream(torch.cuda.current_stream())
    m.set_batch_dev(x.detach(), batch["tokens"], batch["lens"], batch["labels"])
    m.zero_grads()
    logits, dopred, attprob = autograd.step(m, hop_w=f32(HOP_W), feats=x)
    (logits.sum() * 0.0).backward()          # hop_w's criterion alone
    torch.cuda.synchronize()
    assert np.array_equal(x.grad.cpu().numpy().view(np.uint32), m.feature_grad().view(np.uint32))
    assert np.any(x.grad.cpu().numpy())
    m.close()


# ------------------------------------------------------------------------------------------ 6. captured step
def test_captured_step_and_its_key():
    sh, batch, params, _ = problem(8, 49)
    x1, x2 = special_maps(3, 8, 49, seed=31), special_maps(3, 8, 49, seed=37)
    eager = make_model(sh, params)
    eager.normalize_features(eps=EPS)
    refs = []
    for x in (x1, x2):
        put(eager, batch, feats=x)
        refs.append((run_step(eager), eager.norm_feats()[0]))
    eager.close()
    m = make_model(sh, params)
    put(m, batch, feats=x1)
    off = run_step(m, graph=True)             # captured with the switch off ...
    assert not np.array_equal(off["logits"], refs[0][0]["logits"])
    m.normalize_features(eps=EPS)             # ... is not what runs once it is on
    put(m, batch, feats=x1)
    assert_same(run_step(m, graph=True), refs[0][0], "captured, switch on")
    assert np.array_equal(m.norm_feats()[0].view(np.uint32), refs[0][1].view(np.uint32))
    put(m, batch, feats=x2)                   # new maps in the slot: the replay normalises those
    assert_same(run_step(m, graph=True), refs[1][0], "replay on new maps")
    assert np.array_equal(m.norm_feats()[0].view(np.uint32), refs[1][1].view(np.uint32))
    # another eps is another step
    m.normalize_features(eps=0.5)
    put(m, batch, feats=x2)
    other = run_step(m, graph=True)
    assert not np.array_equal(other["logits"], refs[1][0]["logits"])
    m.close()


# ------------------------------------------------------------------------------------------ 7. state
def launches(m):
    return {n: v["launches"] for n, v in m.prof().items() if v["launches"]}


def test_state_rules():
    sh, batch, params, _ = problem(8, 49)
    m = make_model(sh, params)
    lib, h = m._lib, m._h
    assert m.features_normalized == (L.XNORM_NONE, pytest.approx(1e-12))
    xn, nrm, pitch, rows = C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
    dev = lambda: lib.rau_norm_feats_dev(h, C.byref(xn), C.byref(nrm), C.byref(pitch), C.byref(rows))
    assert dev() == STATE                                           # off
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.rau_set_feat_norm(h, L.XNORM_L2, bad) == INVALID
    assert lib.rau_set_feat_norm(h, 7, 1e-3) == INVALID
    assert m.features_normalized[0] == L.XNORM_NONE
    m.normalize_features(eps=EPS)
    assert m.features_normalized == (L.XNORM_L2, pytest.approx(EPS))
    assert dev() == STATE                                           # on, no forward yet
    assert lib.rau_get_norm_feats(h, None, None) == STATE
    put(m, batch)
    m.set_dropout_seed(7, 3)
    m.forward()
    assert dev() == 0 and rows.value == 3 and pitch.value == 52
    m.normalize_features(eps=EPS)                                   # the same again: nothing changes
    assert dev() == 0
    hop_w = f32(HOP_W)
    m.normalize_features(eps=2 * EPS)                               # a change drops the forward
    assert lib.rau_backward(h, hop_w.ctypes.data) == STATE and dev() == STATE
    with pytest.raises(L.RauError):
        m.step_stats()                                              # no statistics either
    m.forward()
    L.check(lib.rau_backward(h, hop_w.ctypes.data))
    m.normalize_features(False)
    assert m.features_normalized[0] == L.XNORM_NONE and dev() == STATE
    m.close()


def test_the_switch_survives_set_batch_size():
    sh, batch, params, _ = problem(8, 49, B=5)
    small = {"feats": batch["feats"][:3], "tokens": np.ascontiguousarray(batch["tokens"][:, :3]),
             "lens": batch["lens"][:3], "labels": batch["labels"][:3]}
    sh3, _, _, _ = problem(8, 49)
    fresh = make_model(sh3, params)
    fresh.normalize_features(eps=EPS)
    put(fresh, small)
    ref = run_step(fresh)
    fresh.close()
    m = make_model(sh, params)
    m.normalize_features(eps=EPS)
    put(m, batch)
    run_step(m)
    m.set_batch_size(3)
    assert m.features_normalized == (L.XNORM_L2, pytest.approx(EPS))
    put(m, small)
    assert_same(run_step(m), ref, "after set_batch_size")
    m.close()


def test_profile_lists_the_launches():
    sh, batch, params, _ = problem(8, 49)
    stored = as_type(special_maps(3, 8, 49), "f16")
    m = make_model(sh, params)
    m.want_feature_grad()
    m.evaluate()                          # no mask: a 16-bit batch is widened by a pass of its own ...
    put(m, batch, feats=stored, feat_type="f16")
    m.prof_enable()
    m.zero_grads(); m.forward(); m.backward(f32(HOP_W)); m.sync()
    off = launches(m)
    assert "l2norm_features" not in off and "l2norm_backward" not in off and off.get("widen_features") == 1
    m.prof_reset()
    m.prof_enable(False)
    m.normalize_features(eps=EPS)         # ... which the normalisation replaces
    put(m, batch, feats=stored, feat_type="f16")
    m.prof_enable()
    m.zero_grads(); m.forward(); m.backward(f32(HOP_W)); m.sync()
    on = launches(m)
    assert on.get("l2norm_features") == 1 and on.get("l2norm_backward") == 1 and "widen_features" not in on
    m.prof_reset()
    m.want_feature_grad(False)
    m.training()
    put(m, batch, feats=stored, feat_type="f16")
    m.set_dropout_seed(7, 3)
    m.zero_grads(); m.forward(); m.backward(f32(HOP_W)); m.sync()
    train = launches(m)
    assert train.get("l2norm_features") == 1 and "l2norm_backward" not in train and "widen_features" not in train
    m.prof_enable(False)
    m.close()
