"""Per-sample region counts on the GPU (rau_set_regions): sample b attends to its first n[b] positions only.

1. parity      against tests/regions_ref.py (one run of the unchanged fp64 oracle per sample, attbymemory's bias at
               -1e30 behind the count): tests/test_gpu_parity.py's 1e-4 max-norm relative bar on every output and
               every layer's gradient, train and evaluate mode, in each of the three forward attention kernels;
2. identity    no counts == counts all S, bit for bit; a run without counts launches what the parent commit did;
3. bias        a uniform count == no counts with the bias at -1e30 behind it, bit for bit (f32 and bf16 mode);
4. garbage     features at masked positions influence nothing;
5. rows        row b of a mixed batch == row b of a batch where every sample has n[b];
6. uploads     plain, typed, image-table, bank and asynchronous batches agree bit for bit;
7. lifetime    of the counts in the two slots;  8. graph_step;  9. module level;  10. errors.
"""
import functools

import numpy as np
import pytest

from rau_vqa_amd import feat16
from tests import regions_ref, util
from tests.test_gpu_att_variants import SEVEN, WIDE

pytestmark = pytest.mark.gpu

TOL = 1e-4
STATE, INVALID = -3, -1
BITS = ("losses", "argmax", "logits", "dopred", "att", "q", "att_c", "att_h", "g_embed", "g_rnn", "g_mult")

BOXES = dict(B=8, T=5, V=40, E=8, Rq=16, D=24, S=100, M=40, A=20, R=16, K=12, H=3)   # box features at a fixed S
# above 400 positions: the fused family's bound at these widths' class (900), the split family's (4096)
SHAPES = {"small": (util.SMALL, 0.5), "seven": (SEVEN, 0.5), "wide": (WIDE, 0.3), "boxes": (BOXES, 0.5),
          "boxes900": (dict(BOXES, S=900), 0.5), "boxes4096": (dict(BOXES, S=4096), 0.5)}


def counts_of(name):
    """Counts with 1, S and values that are no multiple of 4 (seven: 49 = S, 48 = the last full quad, 1)."""
    if name == "small":
        return np.array([12, 7, 3, 1, 5, 12, 2, 9], np.int32)
    if name == "seven":
        return np.array([49, 48, 1, 17, 30, 5], np.int32)
    if name == "boxes":
        return np.array([100, 10, 99, 36, 1, 57, 64, 100], np.int32)
    if name in ("boxes900", "boxes4096"):
        # S, S - 1, 1; the first position of the second and third q0 trip's quad; a count in the last trip
        S = SHAPES[name][0]["S"]
        return np.array([S, 10, S - 1, 257, 1, 513, S - 130, S], np.int32)
    n = np.random.default_rng(11).integers(1, WIDE["S"] + 1, WIDE["B"]).astype(np.int32)
    n[:6] = [196, 1, 195, 7, 64, 129]
    return n


def make(dims, dtype="f32", seed=123, scale=0.5):
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, seed=seed, scale=scale)
    m = RAU(Config(**dims, dtype=dtype))
    m.set_params(params)
    return m, sh, batch, params, masks


def set_mode(m, mode, masks):
    if mode == "train":
        m.training()
        m.set_masks(masks)
    else:
        m.evaluate()


def results(m, hop_w, graph=False, backward=True):
    """One step on the resident batch: every output and gradient."""
    if graph:
        m.graph_step(hop_w, zero_grads=True)
        out = m.outputs()
    else:
        m.zero_grads()
        m.forward()
        out = m.outputs()
        if backward:
            m.backward(hop_w)
    g = m.get_grads()
    out.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]})
    return out


def run(m, batch, mode, masks, hop_w, regions=None, graph=False, **kw):
    set_mode(m, mode, masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], regions=regions, **kw)
    return results(m, hop_w, graph)


def assert_same_bits(a, b, keys=BITS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def differs(a, b):
    return not np.array_equal(a["logits"], b["logits"])


def assert_masked(att, n, positive=True):
    for b, nb in enumerate(n):
        assert np.all(att[:, b, nb:] == 0), b
        assert not positive or np.all(att[:, b, :nb] > 0), b


def hop_weights(sh):
    return np.full(sh.H, float(sh.H), np.float32)


# ---------------------------------------------------------------- 1. parity
@functools.lru_cache(maxsize=None)
def reference(name, mode):
    dims, scale = SHAPES[name]
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    return regions_ref.step(sh, params, batch, masks if mode == "train" else None, hop_weights(sh), counts_of(name))


FUSED, REGS, SPLIT = "att_fwd_fused", "att_fwd_fused_regs", "att_fwd_split"
CASES = [
    ("small", {}, SPLIT),                                                  # up to 64 samples: the split family
    ("small", {"RAU_ATT_SPLIT": "1"}, SPLIT),                              # k_att_ctx
    ("small", {"RAU_ATT_FUSED": "1"}, FUSED),                              # k_att_fwd_dma
    ("small", {"RAU_ATT_FUSED": "1", "RAU_ATT_DMA_OFF": "1"}, REGS),       # k_att_fwd_fused
    ("seven", {"RAU_ATT_SPLIT": "1"}, SPLIT),
    ("seven", {"RAU_ATT_FUSED": "1"}, FUSED),
    ("seven", {"RAU_ATT_FUSED": "1", "RAU_ATT_DMA_OFF": "1"}, REGS),
    ("wide", {}, FUSED),                                                   # above 64 samples: the fused family
    ("wide", {"RAU_ATT_SPLIT": "1"}, SPLIT),
    ("wide", {"RAU_ATT_DMA_OFF": "1"}, REGS),
    ("boxes", {}, SPLIT),
    ("boxes", {"RAU_ATT_FUSED": "1"}, FUSED),
    ("boxes", {"RAU_ATT_FUSED": "1", "RAU_ATT_DMA_OFF": "1"}, REGS),
    ("boxes900", {"RAU_ATT_FUSED": "1"}, REGS),                            # above 256 positions: k_att_fwd_fused
    ("boxes4096", {}, SPLIT),                                              # k_att_ctx over 16 trips of `s += 256`
]


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name,env,kernel", CASES,
                         ids=[n + "".join(" " + k[8:] for k in e) for n, e, _ in CASES])
def test_parity_with_the_per_sample_reference(monkeypatch, name, env, kernel, mode):
    for k in ("RAU_ATT_SPLIT", "RAU_ATT_FUSED", "RAU_ATT_DMA_OFF", "RAU_ATT_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)               # read when the context is created / at every launch
    dims, scale = SHAPES[name]
    n = counts_of(name)
    ref = reference(name, mode)
    m, sh, batch, params, masks = make(dims, scale=scale)
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    assert regions_ref.bias_slice(sh, layouts["mult"]) == regions_ref.bias_slice(sh)
    m.prof_enable()
    got = run(m, batch, mode, masks, hop_weights(sh), regions=n)
    m.sync()
    launched = {k: v["launches"] for k, v in m.prof().items() if k.startswith("att_fwd")}
    m.close()
    assert launched == {kernel: sh.H}, launched
    assert_masked(got["att"], n)
    errs = {k: util.rel_err(got[k], ref[k]) for k in util.OUT_KEYS}
    for grp in ("embed", "rnn", "mult"):
        for lname, sl in util.layer_slices(layouts[grp]):
            r = ref["g_" + grp][sl]
            d = got["g_" + grp][sl]
            errs[lname] = float(np.max(np.abs(d - r))) if np.max(np.abs(r)) < 1e-12 else util.rel_err(d, r)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"
    ok, decided, total = util.argmax_margin_ok(ref["logits"], got["argmax"], ref["argmax"])
    assert ok, "argmax mismatch on a decided row"


# ---------------------------------------------------------------- 2. no counts == counts all S
# rau_prof_entry's listing (class: launches) of zero_grads + forward + backward on a batch WITHOUT counts,
# recorded from the parent commit's library at these shapes, train mode, explicit masks.
PARENT_LAUNCHES = {
    "small": {"apply_mask": 1, "att_bwd_split": 3, "att_fwd_split": 3, "ce_fwd": 1, "colsum": 4, "conv_att_dgrad": 1,
              "conv_att_pre": 1, "conv_att_wgrad": 1, "conv_embed_fwd": 1, "conv_embed_wgrad": 1,
              "dq_reduce": 1, "dropout_features": 1, "embed_bwd": 1, "embed_fwd": 1, "enc_h2h_dgrad": 6,
              "enc_h2h_gemm": 6, "enc_i2h_dgrad": 1, "enc_i2h_gemm": 3, "gather_q": 1, "head_dgrad": 2,
              "head_gemm": 2, "lin_reduce": 6, "loss_reduce": 1, "lstm_bwd": 10, "lstm_fwd": 10,
              "q_proj_dgrad": 1, "q_proj_gemm": 2, "scale_hops": 1, "small_gemm": 27, "transpose": 2,
              "wgrad_gemm": 2},
    "wide": {"apply_mask": 1, "att_bwd_fused": 3, "att_fwd_fused": 3, "ce_fwd": 3, "colsum": 5, "conv_att_dgrad": 3,
             "conv_att_pre": 3, "conv_att_wgrad": 3, "conv_embed_fwd": 3, "conv_embed_wgrad": 3,
             "dq_reduce": 1, "dropout_features": 1, "embed_bwd": 1, "embed_fwd": 1, "enc_h2h_dgrad": 6,
             "enc_h2h_gemm": 6, "enc_i2h_dgrad": 1, "enc_i2h_gemm": 1, "gather_q": 1, "head_dgrad": 6,
             "head_gemm": 6, "lin_reduce": 6, "loss_reduce": 1, "lstm_bwd": 10, "lstm_fwd": 10,
             "q_proj_dgrad": 1, "q_proj_gemm": 1, "scale_hops": 1, "small_gemm": 27, "transpose": 2,
             "wgrad_gemm": 2},
}


@pytest.mark.parametrize("name", ["small", "wide"])
def test_no_counts_is_counts_all_S_and_launches_what_it_did(name):
    dims, scale = SHAPES[name]
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    m.prof_enable()
    plain = run(m, batch, "train", masks, hop_w)
    m.sync()
    listing = {k: v["launches"] for k, v in m.prof().items()}
    m.prof_enable(False)
    assert not m.batch_regions()
    full = run(m, batch, "train", masks, hop_w, regions=np.full(sh.B, sh.S, np.int32))
    assert m.batch_regions()
    assert_same_bits(plain, full)
    assert_same_bits(run(m, batch, "eval", masks, hop_w),
                     run(m, batch, "eval", masks, hop_w, regions=np.full(sh.B, sh.S, np.int32)))
    m.close()
    print(listing)
    assert listing == PARENT_LAUNCHES[name]


# ---------------------------------------------------------------- 3. uniform count == bias at -1e30
@pytest.mark.parametrize("name,n,dtype,mode", [("small", 7, "f32", "train"), ("small", 7, "bf16", "train"),
                                               ("small", 1, "f32", "eval"), ("seven", 48, "f32", "train"),
                                               ("seven", 30, "bf16", "eval")])
def test_uniform_count_is_the_bias_at_minus_1e30(name, n, dtype, mode):
    dims, scale = SHAPES[name]
    m, sh, batch, params, masks = make(dims, dtype=dtype, scale=scale)
    hop_w = hop_weights(sh)
    free = run(m, batch, mode, masks, hop_w)
    counted = run(m, batch, mode, masks, hop_w, regions=np.full(sh.B, n, np.int32))
    biased = regions_ref.masked_params(sh, params, n, m.layout("mult"), dtype=np.float32)
    m.set_params(biased)
    by_bias = run(m, batch, mode, masks, hop_w)
    m.close()
    assert_same_bits(counted, by_bias)
    assert_masked(counted["att"], [n] * sh.B)
    assert differs(counted, free)


# ---------------------------------------------------------------- 4. garbage at masked positions
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["small", "seven"])
def test_features_at_masked_positions_influence_nothing(name, dtype):
    dims, scale = SHAPES[name]
    n = counts_of(name)
    m, sh, batch, params, masks = make(dims, dtype=dtype, scale=scale)
    hop_w = hop_weights(sh)
    other = dict(batch, feats=batch["feats"].copy())
    junk = np.random.default_rng(5).uniform(-100, 100, other["feats"].shape).astype(np.float32)
    for b, nb in enumerate(n):
        other["feats"][b, :, nb:] = junk[b, :, nb:]
    for mode in ("train", "eval"):
        assert_same_bits(run(m, batch, mode, masks, hop_w, regions=n), run(m, other, mode, masks, hop_w, regions=n))
    assert differs(run(m, batch, "eval", masks, hop_w), run(m, other, "eval", masks, hop_w))   # without counts it matters
    m.close()


# ---------------------------------------------------------------- 5. rows are independent
def test_a_row_of_a_mixed_batch_is_the_row_of_a_uniform_one():
    dims, scale = SHAPES["small"]
    n = counts_of("small")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    mixed = run(m, batch, "eval", masks, hop_w, regions=n)
    for nb in np.unique(n):
        uni = run(m, batch, "eval", masks, hop_w, regions=np.full(sh.B, nb, np.int32))
        for b in np.flatnonzero(n == nb):
            for k in ("logits", "att", "argmax"):
                assert np.array_equal(mixed[k][:, b], uni[k][:, b]), (k, b)
    m.close()


# ---------------------------------------------------------------- 6. every upload path
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_every_upload_path_agrees_bit_for_bit(mode):
    from rau_vqa_amd.model import regions_of
    dims, scale = SHAPES["small"]
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    # five images, shared by the eight questions; values every element type holds exactly
    N = 5
    image_of = np.array([0, 1, 2, 0, 1, 3, 4, 4], np.int32)
    n_image = np.array([12, 7, 3, 1, 10], np.int32)
    codes = feat16.fp8_bits(batch["feats"][:N], "e4m3")
    table = feat16.widen(codes, "e4m3")
    n = regions_of(n_image, image_of)
    assert n.tolist() == [12, 7, 3, 12, 7, 1, 10, 10]
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    set_mode(m, mode, masks)

    def step():   # (the evaluate-mode forward of a table batch has no backward: its gradients stay the zeros)
        return results(m, hop_w, backward=mode == "train")
    m.set_batch(np.ascontiguousarray(table[image_of]), *tok, regions=n)
    plain = step()
    assert_masked(plain["att"], n)
    m.set_batch(np.ascontiguousarray(table[image_of]).astype(np.float16), *tok, regions=n)
    assert_same_bits(plain, step())
    m.set_batch(np.ascontiguousarray(codes[image_of]), *tok, feat_type="e4m3", regions=n)
    assert_same_bits(plain, step())
    m.set_batch(table, *tok, image_of=image_of, regions=n_image)            # per-image counts, gathered by the host
    assert m.batch_images() == N and m.batch_regions()
    assert_same_bits(plain, step())
    m.bank_create(N + 2)
    m.bank_put(1, table)
    m.set_batch(None, *tok, bank_rows=np.arange(1, N + 1), image_of=image_of, regions=n_image)
    assert_same_bits(plain, step())
    # asynchronous slots: the counts go between set_batch_async and use_batch
    m.set_batch_async(1, np.ascontiguousarray(table[image_of]), *tok)
    m.set_regions(n, slot=1)
    m.use_batch(1)
    assert m.batch_regions()
    assert_same_bits(plain, step())
    m.set_batch_async(0, table, *tok, image_of=image_of, regions=n_image)
    m.use_batch(0)
    assert_same_bits(plain, step())
    m.set_batch_async(1, None, *tok, bank_rows=np.arange(1, N + 1), image_of=image_of, regions=n_image)
    m.use_batch(1)
    assert_same_bits(plain, step())
    m.close()


# ---------------------------------------------------------------- 7. lifetime
def test_lifetime_of_the_counts_in_the_two_slots():
    dims, scale = SHAPES["small"]
    n = counts_of("small")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    args = (batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    free = run(m, batch, "eval", masks, hop_w)
    counted = run(m, batch, "eval", masks, hop_w, regions=n)
    assert differs(free, counted)
    assert m.batch_regions()
    m.set_batch(*args)                                         # a re-upload into the slot clears them
    assert not m.batch_regions()
    assert_same_bits(free, results(m, hop_w))
    m.set_regions(n)
    assert m.batch_regions()
    assert_same_bits(counted, results(m, hop_w))
    m.set_batch_size(sh.B - 1)                                 # ... and so does set_batch_size
    assert not m.batch_regions()
    m.set_batch_size(sh.B)
    m.evaluate()
    m.set_batch_async(1, *args, regions=n)
    m.use_batch(1)
    m.set_batch_async(0, *args)                                # an upload into the other slot leaves them
    assert m.batch_regions()
    assert_same_bits(counted, results(m, hop_w))
    m.use_batch(0)                                             # a batch without counts
    assert not m.batch_regions()
    assert_same_bits(free, results(m, hop_w))
    m.use_batch(1)                                             # slot 1 still holds its counts
    assert m.batch_regions()
    assert_same_bits(counted, results(m, hop_w))
    m.set_batch_async(1, *args)                                # re-filled in place: gone
    assert not m.batch_regions()
    assert_same_bits(free, results(m, hop_w))
    m.close()


# ---------------------------------------------------------------- 8. graph_step
def test_graph_step_keys_its_cache_by_the_counts():
    dims, scale = SHAPES["small"]
    n = counts_of("small")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)
    eager0 = run(m, batch, "train", masks, hop_w)
    eager = run(m, batch, "train", masks, hop_w, regions=n)
    eager2 = run(m, batch, "train", masks, hop_w, regions=n[::-1].copy())
    assert differs(eager, eager0) and differs(eager, eager2)
    # captured without counts first: a batch with them must not replay that graph
    assert_same_bits(eager0, run(m, batch, "train", masks, hop_w, graph=True))
    assert_same_bits(eager, run(m, batch, "train", masks, hop_w, regions=n, graph=True))
    assert_same_bits(eager2, run(m, batch, "train", masks, hop_w, regions=n[::-1].copy(), graph=True))   # replay: other values
    assert_same_bits(eager0, run(m, batch, "train", masks, hop_w, graph=True))
    assert_same_bits(eager, run(m, batch, "train", masks, hop_w, regions=n, graph=True))
    m.close()


# ---------------------------------------------------------------- 9. module level
def test_multimodal_clone_takes_counts_and_its_backward_needs_none():
    import torch
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda, grad_errs, make_model
    name = "seven"                                             # pitched: attprob and d_X are re-pitched on the way out
    dims, scale = SHAPES[name]
    n = counts_of(name)
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    hop_w = hop_weights(sh)
    ref = reference(name, "train")
    m = make_model(sh, params, masks)
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    feats, y = cuda(batch["feats"]), cuda(batch["labels"], torch.int32)
    n_dev = cuda(n, torch.int32)
    m.zero_grads()
    losses, answers = modules.feval(m, feats, cuda(batch["tokens"], torch.int32), cuda(batch["lens"], torch.int32),
                                    y, hop_w, regions=n_dev)
    m.sync()
    errs = grad_errs(m.get_grads(), ref, layouts)
    errs["losses"] = util.rel_err(losses.numpy(), ref["losses"])
    # one clone by itself, hop 0 from the zero state: outputs against the reference, d_X at masked positions
    ext = torch.cuda.ExternalStream(m.stream(), device=feats.device)
    with torch.cuda.stream(ext):
        q = cuda(ref["q"].astype(np.float32))
        mm = modules.MultimodalClone(m, 0)
        lg, dp, att, cn, hn = mm.forward(q, feats, None, None, regions=n_dev)
        got = {"logits": lg.cpu().numpy(), "att": att.cpu().numpy()}
        dl = modules.CriterionClone(m, 0).backward(lg, y, 1.0)
        d_att = torch.ones_like(att)                            # a gradient at attprob that is NOT zero where a is
        _, dX, _, _ = mm.backward(q, feats, None, None, dl, None, d_att, None, None, want_dX=True)
        dX = dX.cpu().numpy()
    m.sync()
    for k, v in got.items():
        errs["hop0 " + k] = util.rel_err(v, ref[k][0])
    assert_masked(got["att"][None], n)
    for b, nb in enumerate(n):
        assert np.all(dX[b, :, nb:] == 0), b
        assert np.any(dX[b, :, :nb] != 0), b
    # the clamp: counts in device memory outside [1, S] act as 1 and S
    with torch.cuda.stream(ext):
        wild = n_dev.clone()
        wild[0], wild[2] = 10 ** 6, -5
        att2 = mm.forward(q, feats, None, None, regions=wild)[2].cpu().numpy()
    assert np.array_equal(att2, got["att"])                     # n[0] = 49 = S, n[2] = 1
    # the step-level results of the same counts: attention() and merged() show zeros at the masked positions
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], regions=n)
    m.forward()
    assert_masked(m.attention(), n)
    m.predict()
    assert_masked(m.merged()[1], n, positive=False)
    m.close()
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"module-level calls with counts vs the reference above {TOL}: {bad}"
    ok, _, _ = util.argmax_margin_ok(ref["logits"], answers.cpu().numpy(), ref["argmax"])
    assert ok


# ---------------------------------------------------------------- 10. errors
def test_errors_leave_the_previous_counts_in_force():
    dims, scale = SHAPES["small"]
    n = counts_of("small")
    m, sh, batch, params, masks = make(dims, scale=scale)
    hop_w = hop_weights(sh)

    def rc(a, slot=-1):
        a = np.ascontiguousarray(a, np.int32)
        return m._lib.rau_set_regions(m._h, slot, a.ctypes.data)
    m.evaluate()
    assert rc(n) == STATE                                      # no batch in the slot
    assert rc(n, slot=1) == STATE
    counted = run(m, batch, "eval", masks, hop_w, regions=n)
    zero, over = n.copy(), n.copy()
    zero[3], over[6] = 0, sh.S + 1
    assert rc(zero) == INVALID and rc(over) == INVALID and rc(-n) == INVALID
    assert rc(n, slot=2) == INVALID and m._lib.rau_set_regions(m._h, -1, None) == INVALID
    assert m._lib.rau_batch_regions(m._h, None) == INVALID
    assert m.batch_regions()
    assert_same_bits(counted, results(m, hop_w))               # an unchanged forward
    assert rc(n, slot=1) == STATE                              # the other slot is still empty
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], regions=n)
    m.use_batch(1)
    m.forward()
    assert rc(n, slot=1) == STATE                              # current batch of a forward whose backward has not run
    assert rc(zero, slot=0) == INVALID
    m.backward(hop_w)
    assert rc(n[::-1].copy(), slot=1) == 0
    assert differs(counted, results(m, hop_w))
    with pytest.raises(ValueError):
        m.set_regions(n[:-1])
    m.close()
