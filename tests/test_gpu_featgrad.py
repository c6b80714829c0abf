"""The feature-map gradient of the step-level backward on the GPU (rau_set_feat_grad, xgrad.hip, rau_set_batch_dev,
autograd.step(feats=x)).

The oracle is tests/featgrad_ref.py: att_ref._forward restated in fp64 autograd with the maps as a leaf.  The whole
dX is compared with util.rel_err: f32 rows at TOL = 1e-4 (the project's gradient tolerance), bf16 rows at the derived
bar of tests/test_gpu_bf16.py (TOL_BASE + ONE_FLIP + SAFETY x the largest shift of the nudged emulations).

Paths.  The default is the unfused path (GEMM of one hop into a temporary + masked accumulate); RAU_XGRAD_FUSED=1
selects the fused kernel on the shapes it takes (it measured slower in the step: LOG.md).  A context reads the
variable when it is created, and every row creates its own, so the oracle rows run both paths in one process.

Shapes.  X196 reaches the fused kernel with two row tiles (128 + 8 channels), a ragged K tail (M = 72 = 4.5 x 16) and
13 column blocks of which 12 columns are pad; S = 192 is the other side of full column blocks; B = 5 an odd grid for
xcd_remap.  util.SMALL (S = 12) and S = 49 (pitch 52, pad columns) take the unfused path, S = 193 the unfused path
with the mask over the logical tensor on a 196-pitch buffer.
"""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from rau_vqa_amd import feat16
from tests import ext_ref, featgrad_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_select import GROUPS, STATE, TOL, f32, make_model, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X196 = dict(B=6, T=4, V=30, E=8, Rq=16, D=136, S=196, M=72, A=36, R=16, K=12, H=3)
SHAPES = {"X196": X196, "X196_S192": dict(X196, S=192), "X196_B5": dict(X196, B=5), "SMALL": util.SMALL,
          "SMALL_S49": dict(util.SMALL, S=49), "X196_S193": dict(X196, S=193)}
FUSED = {"X196", "X196_S192", "X196_B5"}      # the shapes xgrad_fused_ok takes
HOP_W = [3, 0.5, 2]
_PROBLEMS = {}


# ------------------------------------------------------------------------------------------ machinery
def problem(name):
    if name not in _PROBLEMS:
        sh = util.shapes(SHAPES[name])
        _PROBLEMS[name] = (sh,) + util.make_problem(sh, scale=0.5 if name.startswith("SMALL") else 0.3)
    sh, batch, params, masks = _PROBLEMS[name]
    return sh, dict(batch), params, masks


def counts(sh):
    """COUNTS8-style region counts: full maps, single positions and everything between."""
    return np.minimum(np.array([sh.S, 7, 3, 1, 5, sh.S, 2, 9], np.int32)[:sh.B], sh.S).astype(np.int32)


def put(m, batch, labelled=True, **kw):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"] if labelled else None, **kw)


def dev_step(m, hop_w, out_grads=None, graph=False):
    """One step on the resident batch: (dX [n,D,S], parameter gradients)."""
    if graph:
        m.graph_step(f32(hop_w))
    else:
        m.zero_grads()
        m.forward()
        m.backward(None if hop_w is None else f32(hop_w), out_grads=out_grads)
    return m.feature_grad(), m.get_grads()


def assert_dx(got, ref, what, tol=TOL):
    e = util.rel_err(got, ref)
    print(f"{what}: dX rel_err {e:.2e} (max |dX| {np.max(np.abs(ref)):.2e})")
    assert np.max(np.abs(ref)) > 0
    assert e < tol, f"{what}: {e} >= {tol}"


def seeded_G(H, n, K, S, seed=5):
    rng = np.random.default_rng(seed)
    return {"logits": (rng.normal(size=(H, n, K)) / n).astype(np.float32),
            "dopred": (rng.normal(size=(H, n)) / n).astype(np.float32),
            "attprob": (rng.normal(size=(H, n, S)) / n).astype(np.float32)}


def on_device(G):
    out = {k: torch.as_tensor(np.ascontiguousarray(v, np.float32)).cuda() for k, v in G.items()}
    torch.cuda.synchronize()
    return out


def launches(m):
    return {n: v["launches"] for n, v in m.prof().items() if v["launches"]}


# ------------------------------------------------------------------------------------------ 1. oracle parity
VARIANTS = ("explicit", "philox", "evaluate", "tied", "regions", "trailing_zero", "ce", "ext_only", "bce")
# every shape x every variant on the default path, and again under RAU_XGRAD_FUSED=1 where that reaches the fused
# kernel (evaluate mode and the tied mask hand it dI, not dZ: they stay on the unfused path under either setting)
CASES = [(n, v, "unfused") for n in SHAPES for v in VARIANTS] + \
        [(n, v, "fused") for n in SHAPES if n in FUSED for v in VARIANTS if v not in ("evaluate", "tied")]
# the largest position counts of the two attention families, small widths: the i_embed dgrad over 900 and 4096
# columns per sample and xgrad_accum's rows of that length, with dZ (train), dI (evaluate) and region counts
X900 = dict(B=6, T=4, V=30, E=8, Rq=16, D=40, S=900, M=24, A=20, R=16, K=12, H=3)
SHAPES.update(X900=X900, X4096=dict(X900, S=4096))
CASES += [(n, v, "unfused") for n in ("X900", "X4096") for v in ("explicit", "evaluate", "regions")]


@pytest.fixture
def path(request, monkeypatch):
    monkeypatch.setenv("RAU_XGRAD_FUSED", "1" if request.param == "fused" else "0")
    return request.param


@pytest.mark.parametrize("name,variant,path", CASES, indirect=["path"])
def test_against_the_oracle(name, variant, path):
    sh, batch, params, masks = problem(name)
    hop_w, ref_kw, put_kw, out_grads, labelled = HOP_W, {}, {}, None, True
    ref_masks = masks
    m = make_model(sh, params, None if variant in ("philox", "evaluate", "tied") else masks)
    m.want_feature_grad()
    assert m.feature_grad_wanted
    if variant == "philox":       # the seeded stream: on dense maps the bits are drawn inside the dropout pass and
        m.set_dropout_seed(7, 3)  # regenerated by the backward; get_mask gives the oracle the same bits
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
        put_kw["regions"] = ref_kw["nreg"] = counts(sh)
    elif variant == "trailing_zero":
        hop_w = [3, 2, 0]
    elif variant == "ce":
        hop_w = [float(sh.H)] * sh.H
    elif variant == "ext_only":
        G = seeded_G(sh.H, sh.B, sh.K, sh.S)
        out_grads, hop_w, labelled = on_device(G), None, False
        ref_kw["F"] = ext_ref.linear_F(G["logits"], G["dopred"], G["attprob"])
    elif variant == "bce":
        m.set_answer_loss("bce")
        ref_kw["loss"] = "bce"
    put(m, batch, labelled, **put_kw)
    m.prof_enable()
    dX, _ = dev_step(m, hop_w, out_grads)
    ls = launches(m)
    m.close()
    # the path taken: the fused kernel where it applies (per-hop f32 dZ), else GEMM + accumulate per hop
    if path == "fused":
        assert "xgrad_accum" not in ls and ls.get("conv_embed_dgrad", 0) >= 1, ls
    else:
        assert ls.get("xgrad_accum", 0) >= 1 and ls["xgrad_accum"] == ls.get("conv_embed_dgrad"), ls
    ref = featgrad_ref.step(sh, params, batch if labelled else dict(batch, labels=None), ref_masks, hop_w, **ref_kw)
    assert_dx(dX, ref["g_feats"], f"{name} {variant} {path}")
    if variant == "regions":
        n = counts(sh)
        assert any(n < sh.S)
        for b in range(sh.B):
            assert not dX[b, :, n[b]:].any(), b      # exactly zero behind each count
            assert dX[b, :, :n[b]].any(), b


@pytest.mark.parametrize("name,path", [("X196", "unfused"), ("X196", "fused"), ("SMALL_S49", "unfused")],
                         indirect=["path"])
def test_tied_dropout_with_seeded_masks(name, path):
    """The one tied mask drawn by the device: on dense maps regenerated by the backward (the hop-0 slice of the
    seeded stream), on pitched maps read from memory.  The oracle gets H copies of get_mask's bits."""
    sh, batch, params, masks = problem(name)
    m = make_model(sh, params)
    m.want_feature_grad()
    m.tie_feature_dropout()
    m.set_dropout_seed(7, 3)
    got = {k: m.get_mask(k) for k in masks}
    assert got["x"].shape == (sh.B, sh.D, sh.S)
    put(m, batch)
    dX, _ = dev_step(m, HOP_W)
    m.close()
    ref_masks = dict(got, x=np.ascontiguousarray(np.broadcast_to(got["x"], (sh.H,) + got["x"].shape)))
    ref = featgrad_ref.step(sh, params, batch, ref_masks, HOP_W)
    assert_dx(dX, ref["g_feats"], f"{name} tied, seeded, {path}")


def test_new_key_between_forward_and_backward_is_refused():
    """Bits drawn inside the forward's dropout pass exist nowhere: a backward under another key would regenerate
    other bits.  Refused with nothing launched; the same key again, or a new forward, runs."""
    sh, batch, params, _ = problem("X196")
    m = make_model(sh, params)
    m.want_feature_grad()
    put(m, batch)
    m.set_dropout_seed(7, 3)
    want, grads = dev_step(m, HOP_W)
    hp = f32(HOP_W)
    m.zero_grads()
    m.forward()
    m.set_dropout_seed(7, 4)
    assert m._lib.rau_backward(m._h, hp.ctypes.data) == STATE and b"rau_set_dropout_seed" in m._lib.rau_last_error()
    assert not any(np.any(g) for g in m.get_grads().values())          # nothing was launched
    m.set_dropout_seed(7, 3)                                            # the forward's key again: its backward runs
    assert m._lib.rau_backward(m._h, hp.ctypes.data) == 0
    assert np.array_equal(m.feature_grad().view(np.uint32), want.view(np.uint32))
    same_bits(m.get_grads(), grads)
    # with the switch off nothing is regenerated and nothing is refused
    m.want_feature_grad(False)
    m.zero_grads()
    m.forward()
    m.set_dropout_seed(7, 4)
    assert m._lib.rau_backward(m._h, hp.ctypes.data) == 0
    m.close()


# ------------------------------------------------------------------------------------------ 2. bf16 mode
def test_bf16_tied_dropout_against_the_exact_oracle():
    """The tied backward rounds dZ once, as a sum over the hops: fewer roundings than the emulation's one per hop, so
    (as in tests/test_gpu_tied.py) only the exact-oracle bar applies: TOL_EXACT_GRAD = 1.5e-2, about 4 x 2^-8 for the
    two chained rounded GEMMs (dS -> dZ, dZ -> dX), of max |dX|."""
    from tests.test_gpu_bf16 import TOL_EXACT_GRAD
    sh = util.shapes(dict(X196, D=256, M=256, B=12))
    batch, params, masks = util.make_problem(sh, scale=0.3)
    tied = dict(masks, x=np.ascontiguousarray(masks["x"][0]))
    m = make_model(sh, params, dtype="bf16")
    m.want_feature_grad()
    m.tie_feature_dropout()
    m.set_masks(tied)
    put(m, batch)
    dX, _ = dev_step(m, HOP_W)
    m.close()
    rep = dict(masks, x=np.ascontiguousarray(np.broadcast_to(tied["x"], (sh.H,) + tied["x"].shape)))
    ref = featgrad_ref.step(sh, params, batch, rep, HOP_W)
    assert_dx(dX, ref["g_feats"], "bf16 tied vs exact", TOL_EXACT_GRAD)



@pytest.mark.parametrize("B", [12, 72])
def test_bf16_mode_against_the_emulated_oracle(B):
    sh = util.shapes(dict(X196, D=256, M=256, B=B))
    batch, params, masks = util.make_problem(sh, scale=0.3)
    m = make_model(sh, params, masks, dtype="bf16")
    m.want_feature_grad()
    put(m, batch)
    m.prof_enable()
    dX, _ = dev_step(m, HOP_W)
    ls = launches(m)
    m.close()
    assert ls.get("xgrad_accum") == sh.H == ls.get("conv_embed_dgrad"), ls     # a fused bf16 tile is not built
    with RT.bf16_emulation():
        emu = featgrad_ref.step(sh, params, batch, masks, HOP_W, bf16=True)["g_feats"]
    flip = 0.0
    for nudge in NUDGES:
        with RT.bf16_emulation(nudge):
            flip = max(flip, util.rel_err(featgrad_ref.step(sh, params, batch, masks, HOP_W, bf16=True)["g_feats"], emu))
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    tol = TOL_BASE + one_flip + SAFETY * flip
    print(f"bf16 B={B}: derived bar {tol:.2e} (nudged shift {flip:.2e})")
    assert_dx(dX, emu, f"bf16 B={B}", tol)


# ------------------------------------------------------------------------------------------ 3. switch contract
@pytest.mark.parametrize("name,path", [("X196", "unfused"), ("X196", "fused"), ("SMALL_S49", "unfused")],
                         indirect=["path"])
def test_parameter_gradients_keep_their_bits_and_dx_is_deterministic(name, path):
    sh, batch, params, masks = problem(name)
    m = make_model(sh, params, masks)
    put(m, batch)
    assert not m.feature_grad_wanted
    m.zero_grads(); m.forward(); m.backward(f32(HOP_W))
    off = m.get_grads()
    m.graph_step(f32(HOP_W))
    off_graph = m.get_grads()
    m.want_feature_grad()
    dX1, on1 = dev_step(m, HOP_W)
    dX2, on2 = dev_step(m, HOP_W)
    dXg, on_graph = dev_step(m, HOP_W, graph=True)
    dXg2, _ = dev_step(m, HOP_W, graph=True)
    same_bits(on1, off)
    same_bits(on2, off)
    same_bits(on_graph, off_graph)
    assert np.array_equal(dX1.view(np.uint32), dX2.view(np.uint32))          # two calls
    assert np.array_equal(dXg.view(np.uint32), dX1.view(np.uint32))          # captured == eager
    assert np.array_equal(dXg2.view(np.uint32), dX1.view(np.uint32))         # a replay
    # the result is overwritten, not accumulated, and zero_grads does not touch it
    m.zero_grads()
    assert np.array_equal(m.feature_grad().view(np.uint32), dX1.view(np.uint32))
    # off again: the step is the one without it, and the old result is not handed out
    m.want_feature_grad(False)
    m.zero_grads(); m.forward(); m.backward(f32(HOP_W))
    same_bits(m.get_grads(), off)
    with pytest.raises(L.RauError):
        m.feature_grad()
    m.close()


@pytest.mark.parametrize("path", ["unfused", "fused"], indirect=True)
def test_seeded_masks_under_graph_replay_follow_the_key(path):
    """The regenerated bits come from the device copy of (seed, step): a replay after set_dropout_seed sees the new
    key, and gives the eager step's bits for it."""
    sh, batch, params, _ = problem("X196")
    m = make_model(sh, params)
    m.want_feature_grad()
    put(m, batch)
    m.set_dropout_seed(7, 3)
    a, _ = dev_step(m, HOP_W, graph=True)
    m.set_dropout_seed(7, 4)
    b, _ = dev_step(m, HOP_W, graph=True)
    c, _ = dev_step(m, HOP_W)
    assert not np.array_equal(a, b)
    assert np.array_equal(b.view(np.uint32), c.view(np.uint32))
    m.close()


def test_unfused_path_in_a_fresh_process_agrees_with_the_fused_kernel(tmp_path, monkeypatch):
    monkeypatch.setenv("RAU_XGRAD_FUSED", "1")
    sh, batch, params, masks = problem("X196")
    m = make_model(sh, params, masks)
    m.want_feature_grad()
    put(m, batch)
    m.prof_enable()
    fused, _ = dev_step(m, HOP_W)
    assert "xgrad_accum" not in launches(m)
    m.close()
    out = str(tmp_path / "dx.npy")
    env = dict(os.environ, RAU_XGRAD_FUSED="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "featgrad_child.py"), "X196", out],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"launches {sh.H} {sh.H}" in r.stdout, r.stdout        # GEMM + accumulate per hop: the knob took effect
    assert_dx(np.load(out), fused, "RAU_XGRAD_FUSED=0 vs fused")
    # the documented summation order made checkable: a context of up to 64 samples runs ONE launch group, so both
    # paths add the hops ascending from +0, each term keep ? G * s_x : 0 rounded once, on the same GEMM tile order
    assert np.array_equal(np.load(out).view(np.uint32), fused.view(np.uint32))


# ------------------------------------------------------------------------------------------ 4. dtype and batch contract
@pytest.mark.parametrize("ft", ["f16", "e4m3"])
def test_narrow_batches_give_the_bits_of_the_widened_f32_batch(ft):
    sh, batch, params, masks = problem("X196")
    narrow = batch["feats"].astype(np.float16) if ft == "f16" else feat16.fp8_bits(batch["feats"], ft)
    wide = feat16.widen(narrow, ft)
    assert wide.dtype == np.float32 and not np.array_equal(wide, batch["feats"])
    m = make_model(sh, params, masks)
    m.want_feature_grad()
    m.set_batch(wide, batch["tokens"], batch["lens"], batch["labels"])
    a, ga = dev_step(m, HOP_W)
    m.set_batch(narrow, batch["tokens"], batch["lens"], batch["labels"], feat_type=ft)
    b, gb = dev_step(m, HOP_W)
    m.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    same_bits(ga, gb)


@pytest.mark.parametrize("name", ["X196", "SMALL_S49"])
def test_set_batch_dev_gives_set_batch_bits(name):
    sh, batch, params, masks = problem(name)
    m = make_model(sh, params, masks)
    m.want_feature_grad()
    put(m, batch)
    a, ga = dev_step(m, HOP_W)
    outs_a = m.outputs()
    x = torch.as_tensor(batch["feats"]).cuda()
    torch.cuda.synchronize()
    m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"])
    b, gb = dev_step(m, HOP_W)
    outs_b = m.outputs()
    # with region counts attached afterwards, as to any batch
    m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"], regions=counts(sh))
    c, _ = dev_step(m, HOP_W)
    put(m, batch, regions=counts(sh))
    d, _ = dev_step(m, HOP_W)
    m.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    same_bits(ga, gb)
    for k in ("logits", "dopred", "att", "losses"):
        assert np.array_equal(outs_a[k], outs_b[k]), k
    assert np.array_equal(c.view(np.uint32), d.view(np.uint32)) and not np.array_equal(c, a)


def test_smaller_batch_gives_the_bits_of_a_context_created_at_n():
    sh, batch, params, masks = problem("X196")
    n = 4
    shn = dataclasses.replace(sh, B=n)
    bn = {"feats": batch["feats"][:n], "tokens": np.ascontiguousarray(batch["tokens"][:, :n]),
          "lens": batch["lens"][:n], "labels": batch["labels"][:n]}
    mn = {k: np.ascontiguousarray(v[:, :n]) for k, v in masks.items()}
    m = make_model(sh, params, masks)
    m.want_feature_grad()
    put(m, batch)
    dev_step(m, HOP_W)                      # the buffer is in use at the capacity first
    m.set_batch_size(n)
    assert m.feature_grad_wanted            # the switch and its buffer survive
    with pytest.raises(L.RauError):
        m.feature_grad()                    # ... the result does not
    m.set_masks(mn)
    put(m, bn)
    a, ga = dev_step(m, HOP_W)
    m.close()
    fresh = make_model(shn, params, mn)
    fresh.want_feature_grad()
    put(fresh, bn)
    b, gb = dev_step(fresh, HOP_W)
    fresh.close()
    assert a.shape == (n, sh.D, sh.S) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    same_bits(ga, gb)


# ------------------------------------------------------------------------------------------ 5. refusals
def test_state_refusals():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    lib, h = m._lib, m._h
    p, pitch = C.c_void_p(), C.c_int32()
    put(m, batch)
    m.zero_grads(); m.forward(); m.backward(f32(HOP_W))
    assert lib.rau_feat_grad_dev(h, C.byref(p), C.byref(pitch)) == STATE            # the switch is off
    assert b"rau_set_feat_grad" in lib.rau_last_error()
    m.want_feature_grad()
    assert lib.rau_feat_grad_dev(h, C.byref(p), C.byref(pitch)) == STATE            # that backward did not form it
    m.forward()
    assert lib.rau_feat_grad_dev(h, C.byref(p), C.byref(pitch)) == STATE            # no backward since the forward
    m.backward(f32(HOP_W))
    assert lib.rau_feat_grad_dev(h, C.byref(p), C.byref(pitch)) == 0 and pitch.value == 12 and p.value
    assert lib.rau_feat_grad_dev(h, None, None) == 0
    # the view is ordered on the ctx's stream, where the backward is still queued: torch's stream joins it with an
    # event before it reads (the call itself synchronises nothing)
    t = m.feature_grad_tensor()
    torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(m.stream()))
    assert tuple(t.shape) == (sh.B, sh.D, sh.S) and np.array_equal(t.cpu().numpy(), m.feature_grad())
    m.forward()
    assert lib.rau_feat_grad_dev(h, C.byref(p), C.byref(pitch)) == STATE            # ... until the next forward
    m.close()


def test_pitched_view_is_strided():
    sh, batch, params, masks = problem("SMALL_S49")
    m = make_model(sh, params, masks)
    m.want_feature_grad()
    put(m, batch)
    dX, _ = dev_step(m, HOP_W)
    t = m.feature_grad_tensor()
    torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(m.stream()))
    assert t.stride() == (sh.D * 52, 52, 1) and np.array_equal(t.cpu().numpy(), dX)
    m.close()


@pytest.mark.parametrize("kind", ["table", "bank"])
def test_shared_maps_are_refused_with_no_gradient_changed(kind):
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    m.want_feature_grad()
    put(m, batch)
    _, before = dev_step(m, HOP_W)
    image_of = (np.arange(sh.B) // 2).astype(np.int32)
    table = np.ascontiguousarray(batch["feats"][:sh.B // 2])
    if kind == "bank":
        m.bank_create(sh.B)
        m.bank_put(0, table)
        m.set_batch(None, batch["tokens"], batch["lens"], batch["labels"], image_of=image_of,
                    bank_rows=np.arange(sh.B // 2, dtype=np.int32))
    else:
        m.set_batch(table, batch["tokens"], batch["lens"], batch["labels"], image_of=image_of)
    m.forward()
    hp = f32(HOP_W)
    assert m._lib.rau_backward(m._h, hp.ctypes.data) == STATE
    assert b"image" in m._lib.rau_last_error()
    assert m._lib.rau_graph_step(m._h, hp.ctypes.data, 0) == STATE
    same_bits(m.get_grads(), before)
    # with the switch off the same batch trains as before
    m.want_feature_grad(False)
    m.forward()
    assert m._lib.rau_backward(m._h, hp.ctypes.data) == 0
    m.close()


# ------------------------------------------------------------------------------------------ 6. autograd.step(feats=x)
@pytest.mark.parametrize("name", ["X196", "SMALL_S49"])
def test_autograd_step_trains_a_linear_in_front_of_the_library(name):
    """A torch Linear over the channels feeds x; the loss is a torch function of the outputs plus hop_w's criterion.
    x.grad and the Linear's weight gradient against the fp64 restatement with the same stage in front."""
    from rau_vqa_amd import autograd
    sh, batch, params, masks = problem(name)
    rng = np.random.default_rng(21)
    W0 = (np.eye(sh.D) + 0.1 * rng.normal(size=(sh.D, sh.D))).astype(np.float32)
    teacher = rng.normal(size=(sh.B, sh.K)).astype(np.float32)

    def my_loss(scores, dps, atts, tch):
        uni = sum(scores) / len(scores)
        kl = -(torch.softmax(tch, 1) * torch.log_softmax(uni, 1)).sum(1).mean()
        return kl + 0.1 * sum(-(a * torch.log(a + 1e-12)).sum(1).mean() for a in atts) + 0.05 * sum(d.mean() for d in dps)

    m = make_model(sh, params, masks)
    m.want_feature_grad()
    lin = torch.nn.Linear(sh.D, sh.D, bias=False).cuda()
    with torch.no_grad():
        lin.weight.copy_(torch.as_tensor(W0))
    raw = torch.as_tensor(batch["feats"]).cuda().requires_grad_(True)
    x = lin(raw.transpose(1, 2)).transpose(1, 2).contiguous()          # [n, D, S]
    x.retain_grad()
    own = torch.cuda.ExternalStream(m.stream())
    own.wait_stream(torch.cuda.current_stream())
    m.set_batch_dev(x.detach(), batch["tokens"], batch["lens"], batch["labels"])
    m.zero_grads()
    logits, dopred, attprob = autograd.step(m, hop_w=f32(HOP_W), feats=x)
    loss = my_loss(list(logits), list(dopred), list(attprob), torch.as_tensor(teacher).cuda())
    loss.backward()
    got_x, got_w, got_raw = x.grad.cpu().numpy(), lin.weight.grad.cpu().numpy(), raw.grad.cpu().numpy()
    got_p = m.get_grads()
    layouts = {k: m.layout(k) for k in GROUPS}
    # feats=None: the function is what it was -- same outputs, same parameter gradients, nothing for x
    m.zero_grads()
    lg2, dp2, at2 = autograd.step(m, hop_w=f32(HOP_W))
    my_loss(list(lg2), list(dp2), list(at2), torch.as_tensor(teacher).cuda()).backward()
    same_bits(m.get_grads(), got_p)
    assert torch.equal(lg2, logits) and torch.equal(at2, attprob)
    m.close()

    Wt = torch.as_tensor(W0, dtype=torch.float64).requires_grad_(True)
    pre = lambda f: torch.einsum("ed,bds->bes", Wt, f)
    F = lambda s, d, a: my_loss(s, d, a, torch.as_tensor(teacher, dtype=torch.float64))
    ref = featgrad_ref.step(sh, params, batch, masks, HOP_W, F=F, pre=pre, pre_params=(Wt,))
    # the gradient at x itself: the same restatement with the stage's OUTPUT as the leaf
    x_np = np.einsum("ed,bds->bes", W0.astype(np.float64), batch["feats"].astype(np.float64))
    ref_x = featgrad_ref.step(sh, params, dict(batch, feats=x_np), masks, HOP_W, F=F)
    assert_dx(got_x, ref_x["g_feats"], f"{name} x.grad")
    assert_dx(got_w, ref["g_pre"][0], f"{name} Linear weight gradient")
    assert_dx(got_raw, ref["g_feats"], f"{name} gradient in front of the Linear")
    from tests.test_gpu_select import grad_errs
    errs = grad_errs(got_p, ref, layouts)
    assert all(v < TOL for v in errs.values()), {k: v for k, v in errs.items() if not v < TOL}
