"""Module-level entry points (rau_embed_* / rau_deeplstm_* / rau_multimodal_* / rau_criterion_*)
at the MODEL'S REAL WIDTHS (reference SS:209-229: E=200, Rq=512, M=512, A=256, R=512, K=1000,
T=26, 14x14 maps), against the fp64 oracle, and against the step-level path at the benchmarked
shapes.

tests/test_gpu_modules.py runs these calls at small widths only, where none of the bulk GEMMs take
their interior-tile code: the unpredicated (FAST) loaders of gemm_core.h need M >= 128, D >= 128 and
S % 28 == 0 together, wgrad_dma needs both row counts multiples of 128 (wgrad_dma_ok), the wide
forward tiling rows that are multiples of 64 (conv_wide_ok), and the split-K counts
(conv_wgrad_splits) only reach their real values at these sizes.  The module-level path also
dispatches differently from the step path (rau_modules.hip): conv_embed_fwd / conv_att_pre run once
per clone with nB = B, train mode runs the UNFUSED conv_att_dgrad + conv_embed_wgrad pair (tanh
factor and i_embed bias row sums in conv_embed_wgrad's SC_DTANH operand loader, on the clone's own
dropped-out map) where the step path takes conv_att_dgrad_dz (conv_dz_fused_ok), every Linear's
weight gradient goes through lin_wgrad -> gemm_tn_acc one clone at a time, and conv_embed_dgrad
(the feature-map gradient d_X) exists only here.

Bar: as test_gpu_parity (1e-4 max-norm relative against fp64, answer indices equal on rows the
reference decides); module path vs step path 1e-5.  The C++ oracle runs at batch 16 only, the
BLAS-backed autograd restatement (oracle/ref_torch.py) everywhere else; each oracle result is
computed once.
"""
import numpy as np
import pytest

import oracle
from rau_vqa_amd import synth
from rau_vqa_amd.model import RAU, Config, hop_weights
from tests import util
from tests.test_gpu_modules import cuda, grad_errs, make_model
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

REAL = dict(T=26, V=14000, E=200, Rq=512, S=196, M=512, A=256, R=512, K=1000, H=8)
GROUPS = ("embed", "rnn", "mult")
# gradients that are zero by construction in feval: out_do_pred gets d_do_pred * 0 (SS:566), and a
# constant shift of every attention score cancels in the softmax (the attscore bias)
ZERO_BY_CONSTRUCTION = ("classifier.out_do_pred.weight", "classifier.out_do_pred.bias",
                        "attbycontent.attscore.bias")


def run_feval(m, batch, hop_w):
    """modules.feval over device copies of the batch; returns (losses, answers [H,B], grads)."""
    import torch
    from rau_vqa_amd import modules
    m.zero_grads()
    losses, answers = modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32),
                                    cuda(batch["lens"], torch.int32),
                                    cuda(batch["labels"], torch.int32), hop_w)
    m.sync()
    return losses.numpy(), answers.cpu().numpy(), m.get_grads()


def run_step(m, batch, hop_w, seed=None):
    """The step-level path on the same ctx; seed = (seed, step) of the device Philox masks."""
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    if seed is not None:
        m.set_dropout_seed(*seed)
    m.zero_grads()
    m.forward()
    out = m.outputs()
    m.backward(hop_w)
    return out, m.get_grads()


def check_against_oracle(sh, batch, ref, losses, answers, grads, layouts):
    errs = grad_errs(grads, ref, layouts)
    errs["losses"] = util.rel_err(losses, ref["losses"])
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"module-level feval vs oracle above {TOL}: {bad}\nall: {errs}"
    ok, decided, total = util.argmax_margin_ok(ref["logits"], answers, ref["argmax"])
    assert ok, "module-level answers differ from the oracle's on a decided row"
    print(f"answers: {decided} of {total} rows decided at a 1e-5 margin, all equal; "
          f"{total - decided} undecided")


def check_against_step(g_mod, g_step):
    for k in GROUPS:
        assert util.rel_err(g_mod[k], g_step[k]) < 1e-5, k


def oracle_feval(sh, seed=123, torch_oracle=True, step_too=True):
    """Module-level feval at shape `sh` (train mode, explicit masks, SS hop weights, ragged lengths)
    against the fp64 oracle, then the step path on the same ctx within 1e-5."""
    batch, params, masks = util.make_problem(sh, seed=seed)
    hop_w = hop_weights("SS", sh.H)
    if torch_oracle:
        from oracle import ref_torch
        ref = ref_torch.step(sh, params, batch["feats"], batch["tokens"], batch["lens"],
                             batch["labels"], masks, hop_w)
    else:
        ref = oracle.step(sh, params, batch["feats"], batch["tokens"], batch["lens"],
                          batch["labels"], masks, hop_w, dtype=np.float64)
    m = make_model(sh, params, masks)
    try:
        layouts = {k: m.layout(k) for k in GROUPS}
        losses, answers, g_mod = run_feval(m, batch, hop_w)
        check_against_oracle(sh, batch, ref, losses, answers, g_mod, layouts)
        if step_too:
            _, g_step = run_step(m, batch, hop_w)
            check_against_step(g_mod, g_step)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------
# configs[0]: the C++ oracle's result is shared by the module-level feval and the Lua shim's route
@pytest.fixture(scope="module")
def config0():
    from oracle import ref_torch
    sh = util.shapes(dict(REAL, B=16, D=512))
    batch, params, masks = util.make_problem(sh)
    hop_w = hop_weights("SS", sh.H)
    # logits do not depend on the labels: label every other row with the answer of one of the hops
    # (the reference's forward alone), so that the accuracy counters are not all zero
    fwd = ref_torch.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], None, masks,
                         backward=False)
    rows = np.arange(0, sh.B, 2)
    batch["labels"][rows] = fwd["argmax"][rows % sh.H, rows]
    ref = oracle.step(sh, params, batch["feats"], batch["tokens"], batch["lens"],
                      batch["labels"], masks, hop_w, dtype=np.float64)
    return sh, batch, params, masks, hop_w, ref


def test_config0_feval_over_module_calls(config0):
    """BASELINE.json configs[0] (Ours_SS, 8 hops, batch 16, 14x14x512) through feval's own loops
    over the module-level ABI.  Reaches, per clone with nB = 16: conv_embed_fwd / conv_att_pre on
    the wide tiling (conv_wide_ok: M = 512 and A = 256 are multiples of 64, 16 samples a multiple of
    4); the unfused train-mode conv_att_dgrad (the 128-row per-sample tiles, conv_sample_ok at
    S = 196) and conv_embed_wgrad on the 28-deep interior SC_DTANH tiles (S % 28 == 0, M = D = 512)
    with its dbi row sums, at conv_wgrad_splits(16, 512, 512) = 16 splits; conv_att_wgrad on
    wgrad_dma (wgrad_dma_ok: 256 and 512 are multiples of 128); every Linear's weight gradient at
    batch 16 through lin_wgrad.  The step path on the same ctx takes the fused conv_att_dgrad_dz
    instead (conv_dz_fused_ok) and groups hops: agreement within 1e-5 ties the two together."""
    sh, batch, params, masks, hop_w, ref = config0
    m = make_model(sh, params, masks)
    try:
        layouts = {k: m.layout(k) for k in GROUPS}
        losses, answers, g_mod = run_feval(m, batch, hop_w)
        check_against_oracle(sh, batch, ref, losses, answers, g_mod, layouts)
        out, g_step = run_step(m, batch, hop_w)
        check_against_step(g_mod, g_step)
        assert util.rel_err(losses, out["losses"]) < 1e-5
    finally:
        m.close()


def test_config0_feval_dev_lua_route(config0):
    """The Lua shim's route (bindings/rau.lua RAU.Tensor) at configs[0]: modules.feval_dev drives the
    same module-level calls as modules.feval with nothing but rau_dev_* glue in between (the
    reference's row-by-row `for k=1,B` copy of the selected states, uni accumulation, first-max
    argmax, correct counts).  No glue op sits inside a gradient sum in a different order (the
    d_q accumulation runs hop H..1 in both, row selection only copies), so the gradients are
    BITWISE those of modules.feval; the kernels are the ones test_config0_feval_over_module_calls
    describes.  Correct counts: equal to the oracle's on every row it decides."""
    from rau_vqa_amd import modules
    from rau_vqa_amd.modules import DevTensor
    sh, batch, params, masks, hop_w, ref = config0
    m = make_model(sh, params, masks)
    try:
        layouts = {k: m.layout(k) for k in GROUPS}
        _, _, g_mod = run_feval(m, batch, hop_w)
        feats = DevTensor.zeros(m, sh.B, sh.D, sh.S).copy(batch["feats"])
        x = [DevTensor.ints(m, batch["tokens"][t]) for t in range(sh.T)]
        y = DevTensor.ints(m, batch["labels"])
        m.zero_grads()
        losses, correct, uni = modules.feval_dev(m, feats, x, batch["lens"], y, hop_w, row_loop=True)
        m.sync()
        g_dev = m.get_grads()
        for k in GROUPS:
            assert np.array_equal(g_dev[k], g_mod[k]), k
        errs = grad_errs(g_dev, ref, layouts)
        errs["losses"] = util.rel_err(np.array(losses), ref["losses"])
        errs["uni"] = util.rel_err(uni.numpy(), ref["logits"].sum(0))
        bad = {k: v for k, v in errs.items() if not v < TOL}
        assert not bad, bad
        srt = np.sort(ref["logits"], axis=-1)
        decided = srt[..., -1] - srt[..., -2] > 1e-5 * np.maximum(1.0, np.abs(srt[..., -1]))
        hit = ref["argmax"] == batch["labels"][None, :]
        for h in range(sh.H):
            lo = int((hit[h] & decided[h]).sum())        # undecided rows may go either way
            assert lo <= correct[h] <= lo + int((~decided[h]).sum()), (h, correct[h], lo)
        print(f"correct counts {correct}; {int((~decided).sum())} undecided rows")
    finally:
        m.close()


def test_resnet_d2048_feval_over_module_calls():
    """Ours_ResNet width D = 2048 (ResNet:38,217), batch 16, 4 hops, against the fp64 autograd
    oracle.  Reaches conv_embed_fwd's K = 2048 reduction on the wide tiling per clone (conv_wide_ok:
    2048 % 8 == 0), conv_embed_wgrad's 2048-column interior SC_DTANH tiles (S % 28 == 0) at
    conv_wgrad_splits(16, 512, 2048) = 8 splits (64 tiles), i.e. a split boundary inside the
    clone's 16 samples."""
    oracle_feval(util.shapes(dict(REAL, B=16, D=2048, H=4)))


def test_b144_feval_over_module_calls():
    """Batch 144, 2 hops, against the fp64 autograd oracle: 144 * 196 = 28224 flattened columns per
    clone (220.5 column tiles of 128: interior tiles plus one ragged edge tile per launch of the
    flattened-column GEMMs), row tiles of 64 with a ragged last one (144 = 2 * 64 + 16) in every
    skinny GEMM over 144 rows (lin_wgrad / gemm_tn_acc with B = 144 as its reduction), conv_wide on 144 = 36 * 4
    samples, and conv_wgrad_splits(144, 512, 512) = 32 -> 5 whole samples per split, 29 splits with
    a short last one (4 samples)."""
    oracle_feval(util.shapes(dict(REAL, B=144, D=512, H=2)))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,S,B,mode", [
    (512, 196, 10, "train"), (512, 196, 10, "eval"),
    (2048, 196, 6, "train"), (2048, 196, 6, "eval"),
    (512, 49, 10, "train"), (512, 49, 10, "eval"),
])
def test_multimodal_clone_every_grad_output_real_widths(D, S, B, mode):
    """One multimodal clone with every gradOutput non-zero and d_X requested, at M = 512, A = 256,
    R = 512, K = 1000, against fp64 autograd through RT.multimodal (same masks in train mode: d_X
    carries the feature-map dropout mask, applied on the dense tensor).
    S = 196: conv_embed_fwd on the wide tiling for 4 * (B // 4) samples (conv_wide_ok) and on
    gemm_core.h's flattened tiles for the other 2 (conv_sample_ok(S, 1) is off); conv_embed_dgrad on the 128-row per-sample
    tiles (conv_sample_ok(S, 8)) with D / 128 full row tiles and K = M = 512; conv_embed_wgrad on the
    interior SC_DTANH tiles (S % 28 == 0) with its dbi row sums.
    S = 49: the pitch-52 re-pitch of X, d_attprob and d_X; every conv GEMM on gemm_core.h's
    flattened 128x128 tiles (B * 52 columns: interior tiles plus a ragged edge), conv_att_dgrad's
    128x128 EPI_OUTER tiles at M = 512, conv_wgrad<32> (52 % 28 != 0)."""
    import torch
    from oracle import ref_torch as RT
    from rau_vqa_amd import modules
    sh = util.shapes(dict(REAL, B=B, D=D, S=S, T=4, V=50, H=2))
    batch, params, masks = util.make_problem(sh, seed=31)
    rng = np.random.default_rng(5)
    h = 1
    q = rng.standard_normal((sh.B, sh.Q)).astype(np.float32) * 0.5
    c0 = rng.standard_normal((sh.B, sh.R)).astype(np.float32) * 0.5
    h0 = np.tanh(rng.standard_normal((sh.B, sh.R))).astype(np.float32) * 0.5
    gouts = [rng.standard_normal(s).astype(np.float32) * 0.3 for s in
             [(sh.B, sh.K), (sh.B,), (sh.B, sh.S), (sh.B, sh.R), (sh.B, sh.R)]]
    # ---- autograd reference in float64
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    flat = t64(params["mult"]).clone().requires_grad_(True)
    Pm = RT._split(flat, RT.mult_specs(sh))
    ins = [t64(q).requires_grad_(True),
           t64(batch["feats"]).reshape(sh.B, sh.D, sh.S, 1).requires_grad_(True),
           t64(c0).requires_grad_(True), t64(h0).requires_grad_(True)]
    mk = (lambda k: torch.as_tensor(masks[k][h])) if mode == "train" else (lambda k: None)
    mx = mk("x")
    outs = RT.multimodal(sh, Pm, ins[0], ins[1], ins[2], ins[3], mk("q"),
                         None if mx is None else mx.reshape(sh.B, sh.D, sh.S, 1), mk("mf"))
    torch.autograd.backward(outs, [t64(g) for g in gouts])
    # ---- the clone
    m = make_model(sh, params, masks, mode)
    try:
        layouts = {"mult": m.layout("mult")}
        m.zero_grads()
        clone = modules.MultimodalClone(m, h)
        ext = torch.cuda.ExternalStream(m.stream())
        with torch.cuda.stream(ext):
            args = [cuda(q), cuda(batch["feats"]), cuda(c0), cuda(h0)]
            got = [t.clone() for t in clone.forward(*args)]
            dq, dX, dc, dh = clone.backward(*args, *[cuda(g) for g in gouts], want_dX=True)
        m.sync()
        errs = {}
        for name, a, b in zip(("logits", "do_pred", "attprob", "c", "h"), got, outs):
            errs[name] = util.rel_err(a.cpu().numpy(), b.detach().numpy())
        for name, a, b in (("d_q", dq, ins[0].grad),
                           ("d_X", dX, ins[1].grad.reshape(sh.B, sh.D, sh.S)),
                           ("d_c", dc, ins[2].grad), ("d_h", dh, ins[3].grad)):
            assert tuple(a.shape) == tuple(b.shape), name
            errs[name] = util.rel_err(a.cpu().numpy(), b.numpy())
        g = m.get_grads()["mult"]
        errs.update(grad_errs({"mult": g}, {"g_mult": flat.grad.numpy()}, layouts))
        bad = {k: v for k, v in errs.items() if not v < TOL}
        assert not bad, f"above {TOL}: {bad}\nall: {errs}"
        if mode == "train":   # dropped feature positions get exactly no gradient
            drop = masks["x"][h].reshape(sh.B, sh.D, sh.S) == 0
            assert drop.any() and np.all(dX.cpu().numpy()[drop] == 0)
    finally:
        m.close()


@pytest.mark.parametrize("B", [16, 37])
def test_deeplstm_and_embed_clones_real_widths(B):
    """One embed clone and one DeepLSTM clone at E = 200, Rq = 512 (Q = 2048, gate width 2048)
    against fp64 autograd, with a repeated token inside the clone (the embedding gradient's
    accumulation order).  Reaches the encoder's gemm_nt / gemm_nn at N = 2048 with K = 200 and 512
    (K = 200 is not a whole number of 32-deep K-steps: the predicated tail), and lin_wgrad's
    gemm_tn_acc with the clone's batch as the reduction: 16 rows, and 37 rows = a ragged row
    tile."""
    import torch
    from oracle import ref_torch as RT
    from rau_vqa_amd import modules
    sh = util.shapes(dict(REAL, B=B, D=64, S=4, M=64, A=32, R=32, K=16, H=1, V=300))
    batch, params, masks = util.make_problem(sh, seed=17)
    rng = np.random.default_rng(9)
    t = 2
    state = rng.standard_normal((sh.B, sh.Q)).astype(np.float32) * 0.5
    gstate = rng.standard_normal((sh.B, sh.Q)).astype(np.float32) * 0.3
    tok = batch["tokens"][t].copy()
    tok[1] = tok[0]   # a repeated token inside one clone: accumulation order
    tok[B - 1] = tok[0]
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    emb = t64(params["embed"]).clone().requires_grad_(True)
    flat = t64(params["rnn"]).clone().requires_grad_(True)
    Pr = RT._split(flat, RT.rnn_specs(sh))
    st = t64(state).requires_grad_(True)
    we = torch.tanh(RT._drop(emb.view(sh.V, sh.E)[torch.as_tensor(tok).long() - 1],
                             torch.as_tensor(masks["we"][t]), sh.p_we))
    out = RT.deep_lstm(sh, Pr, we, st, torch.as_tensor(masks["rnn"][t]))
    out.backward(t64(gstate))
    m = make_model(sh, params, masks)
    try:
        layouts = {k: m.layout(k) for k in ("embed", "rnn")}
        m.zero_grads()
        ext = torch.cuda.ExternalStream(m.stream())
        with torch.cuda.stream(ext):
            e, r = modules.EmbedClone(m, t), modules.DeepLSTMClone(m, t)
            x_t, s_in = cuda(tok, torch.int32), cuda(state)
            we_g = e.forward(x_t)
            so = r.forward(we_g, s_in)
            d_x, d_s = r.backward(we_g, s_in, cuda(gstate))
            e.backward(x_t, d_x)
        m.sync()
        g = m.get_grads()
        errs = {"we": util.rel_err(we_g.cpu().numpy(), we.detach().numpy()),
                "state_out": util.rel_err(so.cpu().numpy(), out.detach().numpy()),
                "d_state": util.rel_err(d_s.cpu().numpy(), st.grad.numpy())}
        errs.update(grad_errs(g, {"g_embed": emb.grad.numpy(), "g_rnn": flat.grad.numpy()}, layouts))
        bad = {k: v for k, v in errs.items() if not v < TOL}
        assert not bad, f"above {TOL}: {bad}\nall: {errs}"
        assert np.max(np.abs(g["mult"])) == 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,D,hop_w", [
    ("configs1", 256, 512, hop_weights("SS", 8)),
    ("configs4_rank", 128, 2048, hop_weights("Full", 8, epoch=20)),
])
def test_benchmarked_shapes_module_level_vs_step(name, B, D, hop_w):
    """No oracle: at the benchmarked shapes (configs[1]: batch 256, 14x14x512, SS weights;
    configs[4] per rank: batch 128, D = 2048, the Full schedule at epoch 20 with hops 4..8 gated
    off) the module-level feval and the step path run on one ctx with the same Philox (seed, step),
    so every clone draws the slices the step path uses.  The two share no launch policy: the step
    path groups hops into conv_wide launches over H*B samples, fuses the attention dgrad with the
    tanh factor (conv_dz_fused_ok) and runs its split-K counts over the group; the module path runs
    per clone with nB = B (conv_wgrad_splits(256, 512, 512) = 32, (128, 512, 2048) = 8), unfused, on
    one stream.  Every gradient group within 1e-5, losses within 1e-5 relative, answers equal on
    every row the step logits decide, and no layer slice left at zero unless it is zero by
    construction."""
    sh = util.shapes(dict(REAL, B=B, D=D))
    batch = synth.make_batch(sh.B, sh.T, sh.V, sh.D, sh.S, sh.K, seed=41, lens="ragged")
    m = RAU(Config(**{k: getattr(sh, k) for k in
                      ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H",
                       "p_we", "p_rnn", "p_q", "p_x", "p_mf")}))
    try:
        m.init_uniform(seed=123)
        m.training()
        layouts = {k: m.layout(k) for k in GROUPS}
        m.set_dropout_seed(91, 4)
        losses, answers, g_mod = run_feval(m, batch, hop_w)
        g_mod = {k: v.copy() for k, v in g_mod.items()}
        out, g_step = run_step(m, batch, hop_w, seed=(91, 4))
        errs = {k: util.rel_err(g_mod[k], g_step[k]) for k in GROUPS}
        errs["losses"] = util.rel_err(losses, out["losses"])
        bad = {k: v for k, v in errs.items() if not v < 1e-5}
        assert not bad, f"module-level vs step path above 1e-5: {bad}"
        ok, decided, total = util.argmax_margin_ok(out["logits"], answers, out["argmax"])
        assert ok, "module-level answers differ from the step path's on a decided row"
        print(f"{name}: {decided} of {total} rows decided at a 1e-5 margin, all equal; "
              f"{total - decided} undecided")
        seen = set()
        for grp in GROUPS:
            for lname, sl in util.layer_slices(layouts[grp]):
                seen.add(lname)
                if lname in ZERO_BY_CONSTRUCTION:
                    continue
                for g, path in ((g_mod, "module"), (g_step, "step")):
                    assert np.max(np.abs(g[grp][sl])) > 0, (path, lname)
        assert set(ZERO_BY_CONSTRUCTION) <= seen
    finally:
        m.close()
