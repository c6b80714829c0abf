"""rau_dtype RAU_BF16 (BASELINE.json configs[2]: "bf16 MFMA gate/classifier GEMMs"): bf16-rounded operands,
f32 accumulation, on the 1x1-conv GEMMs and on every product of the Linear layers (LSTM gates, hop
projections, classifier: forward, input gradient, weight gradient).

Two bars.  (1) Against the autograd restatement with the SAME rounding emulated
(oracle/ref_torch.py bf16=True: every operand of those GEMMs rounded to bfloat16, exact accumulation).
What is left between device and emulation is f32 accumulation order (TOL_BASE) plus the operands whose
f32 value sits so close to a bf16 rounding boundary that the device's own f32 error (~3e-7 relative on
I, dS, dZ; up to ~1e-6 on the recurrent states after 26 + 8 cell steps of fast tanh / sigmoid) decides
the rounding the other way: one such flip changes a product by 2^-8 of its size, which on a 12-channel
or one-position reduction is several 1e-4 of the result (round 2's soak: 5.1e-4 and 7.1e-4 on seeds
855 / 859 against a fixed 5e-4 bar) -- and inside the recurrence a flipped operand moves every later
state by that much, which flips further roundings downstream: device and emulation then differ by a
realisation of the mode's own rounding noise, not by an f32 error.  The bar is therefore DERIVED per
tensor: the emulation is run four more times with every operand within NUDGE (6e-7 and 2e-6, relative)
of a boundary rounded the other way, upwards and downwards (ref_torch.step(bf16_nudge=+-NUDGE): operands
further from a boundary keep their rounding bit for bit; the flips propagate through the emulated
recurrence as they do on the device), and a tensor may differ from the plain emulation by TOL_BASE +
ONE_FLIP + SAFETY x the largest of the four shifts, ONE_FLIP = 2^-8 / sqrt(shortest reduction of the model):
what a single flipped rounding that none of the four runs happens to contain does to a sum of that many
terms (3e-4 at the model's real widths, 1-2e-3 on the 4- to 16-wide layers of the fuzz shapes, where the
soak's only failures were: 1.03-1.53 x the bar without this term).  (2) Against the exact fp64 oracle -- the mode is a precision trade of the size of the
bf16 rounding itself, not a different computation: outputs within 3e-2 of their max norm; every
gradient tensor within TOL_EXACT_GRAD = 1.5e-2 (about 4 x 2^-8: two chained rounded GEMMs) of its
UN-CANCELLED magnitude max(max |g|, max sum_b |g_b|), g_b = sample b's share of the gradient
(ref_torch.step(per_sample_abs=True)).  Round 3 held gradients to 3e-2 of max |g| instead, which
passes or fails by the choice of seed: a gradient that is a near-cancelling sum -- the attbymemory
bias over a 2-position map, whose softmax-Jacobian rows sum to zero -- carries the rounding error of
its TERMS (soak seed 2023: max |g| 1.7e-2 against 2.8 un-cancelled, error 1.9e-3 = 0.113 of the one,
6.6e-4 of the other; tests/test_bf16_bar.py reproduces those numbers without a device: the emulation
alone differs from the exact oracle by that much).  Measured on the committed shapes: <= 5.3e-3.
Answer indices: exact wherever the emulated oracle's top-2 margin is decisive.
"""
import numpy as np
import pytest

from oracle import ref_torch as RT
from tests import util

pytestmark = pytest.mark.gpu

TOL_BASE = 2e-4       # accumulation order alone (measured <= 6e-5 on the committed shapes)
NUDGES = (2e-6, -2e-6, 1e-5, -1e-5)   # 2x the measured f32 error of the rounded intermediates (conv operands; recurrent states)
SAFETY = 5.0          # the device takes its own subset of the flips: another draw of the same noise, not a subset of one run's
TOL_EXACT = 3e-2        # outputs, relative to their max norm
TOL_EXACT_GRAD = 1.5e-2  # gradients, relative to the un-cancelled magnitude (module docstring)


def run(dims, scale, mode="train", lens="ragged", problem=None):
    """problem: a prepared (batch, params, masks) in place of util.make_problem's (tests/range_cases.py)."""
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(dims)
    batch, params, masks = problem or util.make_problem(sh, lens=lens, scale=scale)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    mk = masks if mode == "train" else None
    args = (sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], mk, hop_w)
    emu = RT.step(*args, bf16=True)
    emu_nudged = [RT.step(*args, bf16=True, bf16_nudge=n) for n in NUDGES]
    exact = RT.step(*args, per_sample_abs=True)
    cfg = Config(**{k: getattr(sh, k) for k in
                    ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H",
                     "p_we", "p_rnn", "p_q", "p_x", "p_mf")}, dtype="bf16")
    m = RAU(cfg)
    m.set_params(params)
    if mode == "train":
        m.training()
        m.set_masks(masks)
    else:
        m.evaluate()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.zero_grads()
    m.forward()
    got = m.outputs()
    m.backward(hop_w)
    g = m.get_grads()
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    m.close()
    def tensors(res, grads):
        out = {k: np.asarray(res[k]) for k in util.OUT_KEYS}
        for grp in layouts:
            for name, sl in util.layer_slices(layouts[grp]):
                out[name] = np.asarray(grads[grp][sl])
        return out

    def as_grads(ref):
        return {grp: ref["g_" + grp] for grp in layouts}
    dev = tensors(got, g)
    t_emu, t_ex = (tensors(r, as_grads(r)) for r in (emu, exact))
    t_nudged = [tensors(r, as_grads(r)) for r in emu_nudged]

    def err(a, b):
        return float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    bad, widest, ratio = {}, 0.0, 0.0
    kmin = min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K)
    one_flip = 2.0 ** -8 / np.sqrt(kmin)
    for k in dev:
        flip = max(err(t[k], t_emu[k]) for t in t_nudged)
        tol = TOL_BASE + one_flip + SAFETY * flip
        widest = max(widest, tol)
        e = err(dev[k], t_emu[k])
        ratio = max(ratio, e / tol)
        if not e < tol:
            bad[k] = (e, tol)
    print(f"bf16: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated oracle, (error, derived bar): {bad}"
    # (2) vs the exact oracle: outputs against their max norm, gradients against the un-cancelled
    # magnitude of the batch sum
    t_abs = tensors({k: exact[k] for k in util.OUT_KEYS}, {grp: exact["gabs_" + grp] for grp in layouts})
    bad = {}
    for k in dev:
        if k in util.OUT_KEYS:
            e, tol = err(dev[k], t_ex[k]), TOL_EXACT
        else:
            scale = max(float(np.max(np.abs(t_ex[k]))), float(np.max(t_abs[k])))
            e = float(np.max(np.abs(dev[k] - t_ex[k]))) / scale if scale > 1e-12 else \
                float(np.max(np.abs(dev[k] - t_ex[k])))
            tol = TOL_EXACT_GRAD
        if not e < tol:
            bad[k] = (e, tol)
    assert not bad, f"vs exact oracle, (error, bar): {bad}"
    print(f"bf16: widest derived bar {widest:.2e}")
    ok, _, _ = util.argmax_margin_ok(emu["logits"], got["argmax"], emu["argmax"], margin=5e-3)
    assert ok


def test_bf16_small_train():
    run(util.SMALL, 0.5)


def test_bf16_small_eval():
    run(util.SMALL, 0.5, mode="eval")


def test_bf16_medium_s196_k1000():
    run(util.MEDIUM, 0.2)


def test_bf16_resnet_channels_d2048():
    dims = dict(B=6, T=4, V=40, E=200, Rq=32, D=2048, S=196, M=64, A=32, R=32, K=1000, H=2)
    run(dims, 0.05)


def test_bf16_dgrad16_tile_shapes():
    """14x14 map with M % 128 == 0 and A % 32 == 0: the attention dgrad runs on dgrad16.hip (bf16-rounded
    dS and Wp); two row tiles per sample, odd sample count."""
    dims = dict(B=5, T=4, V=40, E=16, Rq=32, D=64, S=196, M=256, A=64, R=32, K=52, H=2)
    run(dims, 0.1)


def test_bf16_near_cancelling_bias_gradient_soak_seed_2023():
    """The shape of round 3's one un-triaged soak failure (tools/soak_bf16.py seed 2023): a
    2-position map, 82 samples -- the attbymemory bias gradient is a sum of terms that cancel to
    1/170 of their magnitude, so its error relative to max |g| is 0.11 although every term carries
    an ordinary bf16 rounding error.  Held to the bar scaled by the un-cancelled magnitude."""
    dims = dict(B=82, T=1, V=42, E=28, Rq=24, D=32, S=2, M=132, A=80, R=44, K=16, H=3)
    run(dims, 0.3)


def test_bf16_7x7_feature_map_s49():
    dims = dict(B=6, T=5, V=40, E=8, Rq=16, D=24, S=49, M=40, A=20, R=16, K=12, H=3)
    run(dims, 0.5)


def test_f32_results_do_not_depend_on_the_bf16_code_path():
    """dtype f32 stays the exact path: bitwise equal outputs from two f32 contexts, and different
    from the bf16 context's (guards against the flag leaking into the default mode)."""
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(util.SMALL)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    outs = []
    for dt in ("f32", "f32", "bf16"):
        m = RAU(Config(**{k: getattr(sh, k) for k in
                          ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")}, dtype=dt))
        m.set_params(params)
        m.training()
        m.set_masks(masks)
        m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
        m.forward()
        outs.append(m.logits())
        m.close()
    assert np.array_equal(outs[0], outs[1])
    assert not np.array_equal(outs[0], outs[2])


def test_bf16_storage_of_operands_changes_nothing(monkeypatch):
    """On 14x14 maps the bf16 step path keeps the dropped-out feature maps, dZ and the transposed conv
    weights as bf16 IN HBM (rau_ctx.hip: xd16 / WiT16 / WpT16).  Those values are rounded to bf16
    when staged anyway, so every output and gradient must be bitwise what the f32-storage path
    (RAU_XD_F32=1, read when the context is created) produces."""
    from rau_vqa_amd.model import RAU, Config
    dims = dict(B=6, T=4, V=40, E=16, Rq=16, D=96, S=196, M=64, A=32, R=32, K=24, H=3)
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=0.3)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    res = []
    for f32_storage in (True, False):
        if f32_storage:
            monkeypatch.setenv("RAU_XD_F32", "1")
        else:
            monkeypatch.delenv("RAU_XD_F32", raising=False)
        m = RAU(Config(**{k: getattr(sh, k) for k in
                          ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")}, dtype="bf16"))
        m.set_params(params)
        m.training()
        m.set_masks(masks)
        m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
        m.zero_grads()
        m.forward()
        out = m.outputs()
        m.backward(hop_w)
        res.append((out, m.get_grads()))
        m.close()
    for k in util.OUT_KEYS:
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    for grp in ("embed", "rnn", "mult"):
        assert np.array_equal(res[0][1][grp], res[1][1][grp]), grp


# ---------------------------------------------------------------- one clone at a time (given inputs)
# Inside the whole step a flipped rounding moves every later recurrent state, so the bars above are as wide
# as the mode's own rounding noise.  With ONE clone and GIVEN inputs nothing feeds back: the operands that
# can flip are the handful of intermediates inside the cell, each flip is a single event, and the derived
# bar is tight again (CLONE_NUDGES: 2x the f32 error of those intermediates; SAFETY 2 as in round 3).
CLONE_NUDGES = (6e-7, -6e-7, 2e-6, -2e-6)
CLONE_TILES = dict(B=12, T=6, V=60, E=64, Rq=64, D=256, S=196, M=256, A=64, R=64, K=200, H=3)


def _clone_bars(dev, emus):
    """dev / emus[i]: dicts of arrays; emus[0] the plain emulation, the rest nudged."""
    def err(a, b):
        return float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    bad, bars, errs = {}, {}, {}
    for k, v in dev.items():
        flip = max(err(e[k], emus[0][k]) for e in emus[1:])
        bars[k] = TOL_BASE + 2.0 * flip
        errs[k] = err(v, emus[0][k])
        if not errs[k] < bars[k]:
            bad[k] = (errs[k], bars[k])
    assert not bad, f"clone vs emulated oracle, (error, derived bar): {bad}"
    kw = max(bars, key=bars.get)
    return (f"{len(bars)} tensors, median derived bar {np.median(list(bars.values())):.1e}, widest {bars[kw]:.1e} "
            f"({kw}), largest error {max(errs.values()):.1e}")


def _bf16_model(sh, params, masks, mode):
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**{k: getattr(sh, k) for k in
                      ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H",
                       "p_we", "p_rnn", "p_q", "p_x", "p_mf")}, dtype="bf16"))
    m.set_params(params)
    if mode == "train":
        m.training()
        m.set_masks(masks)
    else:
        m.evaluate()
    return m


@pytest.mark.parametrize("dims,scale,mode", [(util.SMALL, 0.5, "train"), (util.SMALL, 0.5, "eval"),
                                             (CLONE_TILES, 0.3, "train")],
                         ids=["small-train", "small-eval", "tiles-train"])
def test_bf16_multimodal_clone_given_inputs(dims, scale, mode):
    """One multimodal clone (SS:292-307) in RAU_BF16 mode, forward and backward with every gradOutput
    non-zero, against the rounding-emulating restatement under autograd."""
    import torch
    from rau_vqa_amd import modules
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    rng = np.random.default_rng(5)
    h = 1
    q = rng.standard_normal((sh.B, sh.Q)).astype(np.float32) * 0.5
    c0 = rng.standard_normal((sh.B, sh.R)).astype(np.float32) * 0.5
    h0 = np.tanh(rng.standard_normal((sh.B, sh.R))).astype(np.float32) * 0.5
    gouts = [rng.standard_normal(s).astype(np.float32) * 0.3 for s in
             [(sh.B, sh.K), (sh.B,), (sh.B, sh.S), (sh.B, sh.R), (sh.B, sh.R)]]
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    mk = (lambda k: torch.as_tensor(masks[k][h])) if mode == "train" else (lambda k: None)
    names_out = ("logits", "do_pred", "attprob", "c", "h")

    def emulate(nudge):
        flat = t64(params["mult"]).clone().requires_grad_(True)
        Pm = RT._split(flat, RT.mult_specs(sh))
        ins = [t64(q).requires_grad_(True), t64(batch["feats"]).reshape(sh.B, sh.D, sh.S, 1),
               t64(c0).requires_grad_(True), t64(h0).requires_grad_(True)]
        mx = mk("x")
        with RT.bf16_emulation(nudge):
            outs = RT.multimodal(sh, Pm, ins[0], ins[1], ins[2], ins[3], mk("q"),
                                 None if mx is None else mx.reshape(sh.B, sh.D, sh.S, 1), mk("mf"), bf16=True)
            torch.autograd.backward(outs, [t64(g) for g in gouts])
        res = {n: o.detach().numpy() for n, o in zip(names_out, outs)}
        res.update(d_q=ins[0].grad.numpy(), d_c=ins[2].grad.numpy(), d_h=ins[3].grad.numpy())
        return res, flat.grad.numpy()

    emus = [emulate(n) for n in (0.0,) + CLONE_NUDGES]
    m = _bf16_model(sh, params, masks, mode)
    layout = m.layout("mult")
    m.zero_grads()
    clone = modules.MultimodalClone(m, h)
    ext = torch.cuda.ExternalStream(m.stream())
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    with torch.cuda.stream(ext):
        args = [cu(q), cu(batch["feats"]), cu(c0), cu(h0)]
        got = clone.forward(*args)
        dq, _, dc, dh = clone.backward(*args, *[cu(g) for g in gouts])
    m.sync()
    dev = {n: a.cpu().numpy() for n, a in zip(names_out, got)}
    dev.update(d_q=dq.cpu().numpy(), d_c=dc.cpu().numpy(), d_h=dh.cpu().numpy())
    g = m.get_grads()["mult"]
    m.close()
    table = []
    for res, gflat in emus:
        d = dict(res)
        for name, sl in util.layer_slices(layout):
            d[name] = gflat[sl]
        table.append(d)
    for name, sl in util.layer_slices(layout):
        dev[name] = g[sl]
    print("bf16 multimodal clone:", _clone_bars(dev, table))


@pytest.mark.parametrize("dims,scale", [(util.SMALL, 0.5), (CLONE_TILES, 0.3)], ids=["small", "tiles"])
def test_bf16_deeplstm_clone_given_inputs(dims, scale):
    """One lstm clone (model/DeepLSTM.lua:14-71) behind its embedding clone in RAU_BF16 mode, forward and
    backward, against the rounding-emulating restatement under autograd."""
    import torch
    from rau_vqa_amd import modules
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    rng = np.random.default_rng(9)
    t = 2
    state = rng.standard_normal((sh.B, sh.Q)).astype(np.float32) * 0.5
    gstate = rng.standard_normal((sh.B, sh.Q)).astype(np.float32) * 0.3
    tok = batch["tokens"][t].copy()
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)

    def emulate(nudge):
        emb = t64(params["embed"]).clone().requires_grad_(True)
        flat = t64(params["rnn"]).clone().requires_grad_(True)
        Pr = RT._split(flat, RT.rnn_specs(sh))
        st = t64(state).requires_grad_(True)
        with RT.bf16_emulation(nudge):
            we = torch.tanh(RT._drop(emb.view(sh.V, sh.E)[torch.as_tensor(tok).long() - 1],
                                     torch.as_tensor(masks["we"][t]), sh.p_we))
            out = RT.deep_lstm(sh, Pr, we, st, torch.as_tensor(masks["rnn"][t]))
            out.backward(t64(gstate))
        return dict(state=out.detach().numpy(), d_state=st.grad.numpy(), g_rnn=flat.grad.numpy(),
                    g_embed=emb.grad.numpy())

    emus = [emulate(n) for n in (0.0,) + CLONE_NUDGES]
    m = _bf16_model(sh, params, masks, "train")
    m.zero_grads()
    ext = torch.cuda.ExternalStream(m.stream())
    cu = lambda a, dt=None: (torch.as_tensor(np.ascontiguousarray(a)).cuda() if dt is None
                             else torch.as_tensor(np.ascontiguousarray(a)).cuda().to(dt))
    with torch.cuda.stream(ext):
        e, r = modules.EmbedClone(m, t), modules.DeepLSTMClone(m, t)
        x_t, s_in = cu(tok, torch.int32), cu(state)
        we_g = e.forward(x_t)
        so = r.forward(we_g, s_in)
        d_x, d_s = r.backward(we_g, s_in, cu(gstate))
        e.backward(x_t, d_x)
    m.sync()
    g = m.get_grads()
    dev = dict(state=so.cpu().numpy(), d_state=d_s.cpu().numpy(), g_rnn=g["rnn"], g_embed=g["embed"])
    m.close()
    print("bf16 deeplstm clone:", _clone_bars(dev, emus))
