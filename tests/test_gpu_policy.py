"""A context runs under the environment it was created in (csrc/policy.h): rau_create parses the
A/B variables once into the context's record, and nothing the context does later -- a launch, a resize, a captured
step -- looks at the environment again.

All three tests change a variable AFTER a context exists, in one process, and read the path taken off the launch
counts of rau_prof_entry.  The dims are the generic ones of tests/knob_check.py at B = 24 (T = 7; up to 64 samples the
chain's non-recurrent GEMMs are split off to the side stream), and shape X196 of tests/test_gpu_featgrad.py.
"""
import numpy as np
import pytest

from oracle import ref_torch
from tests import util
from tests.test_gpu_featgrad import HOP_W, dev_step, launches, problem as x196_problem, put
from tests.test_gpu_select import GROUPS, TOL, grad_errs, make_model

pytestmark = pytest.mark.gpu

DIMS = dict(B=24, T=7, V=120, E=200, Rq=64, D=64, S=196, M=128, A=64, R=64, K=1000, H=4)
_PROBLEM = {}


def problem():
    """The B = 24 problem with a longest question of T = 7 tokens and its fp64 reference step, computed once."""
    if not _PROBLEM:
        sh = util.shapes(DIMS)
        lens = np.array([7, 3, 5, 7, 4, 6] * 4, np.int32)
        batch, params, masks = util.make_problem(sh, lens=lens, scale=0.2)
        hop_w = np.full(sh.H, float(sh.H), np.float32)
        ref = ref_torch.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks, hop_w)
        _PROBLEM.update(sh=sh, batch=batch, params=params, masks=masks, hop_w=hop_w, ref=ref)
    p = _PROBLEM
    return p["sh"], p["batch"], p["params"], p["masks"], p["hop_w"], p["ref"]


def train_step(m, masks, batch, hop_w):
    m.training()
    m.set_masks(masks)
    put(m, batch)
    m.zero_grads()
    m.forward()
    out = m.outputs()
    m.backward(hop_w)
    return out, m.get_grads()


def forward_counts(m, batch, masks=None):
    """Launch counts per class of one forward of `batch`: train mode under `masks`, evaluate mode without."""
    if masks is None:
        m.evaluate()
    else:
        m.training()
        m.set_masks(masks)
    put(m, batch)
    m.prof_enable()
    m.prof_reset()
    m.forward()
    got = launches(m)
    m.prof_enable(False)
    return got


def assert_parity(m, out, grads, ref, what):
    errs = {k: util.rel_err(out[k], ref[k]) for k in util.OUT_KEYS}
    errs.update(grad_errs(grads, ref, {k: m.layout(k) for k in GROUPS}))
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"{what}: relative errors above {TOL}: {bad}"


def test_two_contexts_keep_their_own_environment(monkeypatch):
    """RAU_ENC_CHUNKS: the side stream's layer-1 input projection of tokens 5..TL as 1 launch (context A) or as
    min(4, TL - 4) launches (context B, variable unset), each beside the one launch of the first four tokens."""
    sh, batch, params, masks, hop_w, ref = problem()
    TL = int(batch["lens"].max())
    assert TL == 7
    monkeypatch.setenv("RAU_ENC_CHUNKS", "1")
    a = make_model(sh, params)
    monkeypatch.delenv("RAU_ENC_CHUNKS")
    b = make_model(sh, params)
    assert forward_counts(a, batch)["enc_i2h_gemm"] == 1 + 1
    assert forward_counts(b, batch)["enc_i2h_gemm"] == 1 + min(4, TL - 4) == 4
    assert forward_counts(a, batch)["enc_i2h_gemm"] == 1 + 1      # ... whatever ran in the process in between
    out_a1, g_a1 = train_step(a, masks, batch, hop_w)
    out_b, g_b = train_step(b, masks, batch, hop_w)
    out_a2, g_a2 = train_step(a, masks, batch, hop_w)
    assert np.array_equal(out_a1["logits"].view(np.uint32), out_a2["logits"].view(np.uint32))
    assert_parity(a, out_a2, g_a2, ref, "context A (RAU_ENC_CHUNKS=1)")
    assert_parity(b, out_b, g_b, ref, "context B (unset)")
    a.close()
    b.close()


def test_a_resized_context_keeps_its_record(monkeypatch):
    """RAU_HOP_GROUPS = 1,1,1,1 at H = 4: four conv_embed_fwd launches per train forward where the default partition
    of up to 64 samples is one group.  rau_set_batch_size plans the batch again -- from the record."""
    sh, batch, params, masks, _, _ = problem()
    monkeypatch.setenv("RAU_HOP_GROUPS", "1,1,1,1")
    m = make_model(sh, params)
    assert forward_counts(m, batch, masks)["conv_embed_fwd"] == 4
    monkeypatch.delenv("RAU_HOP_GROUPS")
    m.set_batch_size(16)       # (the profile is off: forward_counts leaves it so)
    m.set_batch_size(sh.B)
    assert forward_counts(m, batch, masks)["conv_embed_fwd"] == 4
    m.close()
    fresh = make_model(sh, params)
    assert forward_counts(fresh, batch, masks)["conv_embed_fwd"] == 1
    fresh.close()


def test_a_captured_step_and_an_eager_step_take_the_same_path(monkeypatch):
    """RAU_XGRAD_FUSED = 1 at creation, 0 afterwards: the captured step and the eager one both run the fused
    feature-map gradient kernel, and give the same bits."""
    sh, batch, params, masks = x196_problem("X196")
    monkeypatch.setenv("RAU_XGRAD_FUSED", "1")
    m = make_model(sh, params, masks)
    m.want_feature_grad()
    monkeypatch.setenv("RAU_XGRAD_FUSED", "0")
    put(m, batch)
    dx_graph, _ = dev_step(m, HOP_W, graph=True)
    m.prof_enable()
    dx_eager, _ = dev_step(m, HOP_W)
    ls = launches(m)
    m.close()
    assert np.array_equal(dx_graph.view(np.uint32), dx_eager.view(np.uint32))
    assert "xgrad_accum" not in ls and ls.get("conv_embed_dgrad", 0) >= 1, ls
