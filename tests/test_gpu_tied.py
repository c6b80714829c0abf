"""Tied feature-map dropout (rau_set_feat_dropout, RAU_XDROP_TIED; RAU.tie_feature_dropout): one mask on the raw
feature map shared by all hops, so a train-mode step runs the two 1x1 convolutions and their three gradients
once, the backward summing the hops first (csrc/tied_bwd.hip).

Tied dropout is per-hop dropout with H equal masks, so the reference is the unchanged fp64 oracle given
masks["x"] = broadcast(m, (H, B, D, S)); where the oracle has no such term (region counts, select / attention /
merged-answer losses) it is the per-hop device path given the replicated mask.  The bar is tests/test_gpu_parity.py's
TOL = 1e-4 on every output and every gradient tensor, with its rule for references that are zero, and answer
indices exact on the rows the reference decides at its 1e-5 margin.  bf16 mode: bar (2) of tests/test_gpu_bf16.py
against the exact oracle, both constants imported.
"""
import functools

import numpy as np
import pytest

import oracle
from tests import util
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

S49 = dict(util.SMALL, S=49)                       # pitch 52: the pitched dropout pass, pad columns in both sums
CFG_KEYS = ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H", "p_we", "p_rnn", "p_q", "p_x", "p_mf")
CONVS = ("conv_embed_fwd", "conv_att_pre", "conv_att_dgrad", "conv_att_wgrad", "conv_embed_wgrad")


def f32(a):
    return np.asarray(a, np.float32)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(shapes, batch, params, masks with x [B, D, S], scale) of a named case, built once."""
    dims, scale, over = {"small": (util.SMALL, 0.5, {}), "edge": (util.EDGE, 0.5, {}),
                         "medium": (util.MEDIUM, 0.2, {}), "s49": (S49, 0.5, {}),
                         "px0": (util.SMALL, 0.5, dict(p_x=0.0)),
                         "b5": (dict(util.SMALL, B=5), 0.5, {}),
                         "s900": (dict(util.SMALL, S=900), 0.5, {})}[name]
    sh = util.shapes(dims, **over)
    batch, params, masks = util.make_problem(sh, scale=scale)
    masks = dict(masks, x=np.ascontiguousarray(masks["x"][0]))   # hop 0's mask is the tied one
    return sh, batch, params, masks


def replicated(sh, masks):
    """The per-hop masks tied dropout stands for: the one x mask for every hop."""
    return dict(masks, x=np.ascontiguousarray(np.broadcast_to(masks["x"], (sh.H,) + masks["x"].shape)))


@functools.lru_cache(maxsize=None)
def oracle_ref(name, hop_w):
    sh, batch, params, masks = problem(name)
    return oracle.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"],
                       replicated(sh, masks), f32(hop_w), dtype=np.float64)


def model(sh, params, tied=True, dtype="f32", cap=None):
    from rau_vqa_amd.model import RAU, Config
    kw = {k: getattr(sh, k) for k in CFG_KEYS}
    if cap:
        kw["B"] = cap
    m = RAU(Config(**kw, dtype=dtype))
    m.set_params(params)
    m.training()
    if tied:
        m.tie_feature_dropout()
    return m


def results(m):
    out = m.outputs()
    g = m.get_grads()
    out.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]})
    return out


def step(m, batch, hop_w, masks=None, graph=False, **loss):
    """One step on the resident-to-be batch; masks None keeps the seeded stream."""
    if masks is not None:
        m.set_masks(masks)
    m.set_batch(**batch)
    if graph:
        m.graph_step(f32(hop_w), **loss)
    else:
        m.zero_grads()
        m.forward()
        m.backward(f32(hop_w), **loss)
    return results(m)


def errors(got, ref, layouts):
    errs = {k: util.rel_err(got[k], ref[k]) for k in util.OUT_KEYS}
    for grp in ("embed", "rnn", "mult"):
        for name, sl in util.layer_slices(layouts[grp]):
            r = np.asarray(ref["g_" + grp][sl], np.float64)
            if np.max(np.abs(r)) < 1e-12:   # a gradient that is zero analytically: absolute
                errs[name] = float(np.max(np.abs(got["g_" + grp][sl] - r)))
            else:
                errs[name] = util.rel_err(got["g_" + grp][sl], r)
    return errs


def assert_close(got, ref, layouts, what):
    errs = errors(got, ref, layouts)
    print(f"{what}: largest error {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"{what}: relative errors above {TOL}: {bad}"
    ok, decided, total = util.argmax_margin_ok(np.asarray(ref["logits"], np.float64), got["argmax"], ref["argmax"])
    assert ok, f"{what}: answer index differs on a decided row"


def assert_same_bits(a, b, what):
    for k in util.OUT_KEYS + ("argmax",) + util.GRAD_KEYS:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def layouts_of(m):
    return {k: m.layout(k) for k in ("embed", "rnn", "mult")}


# ------------------------------------------------------------------ against the fp64 oracle, explicit masks
@pytest.mark.parametrize("name,hop_w", [
    ("small", (3, 3, 3)),        # H 3
    ("edge", (1,)),              # H 1: outer_sum is not launched
    ("medium", (2, 2)),          # S 196: the 14 x 14 kernel classes
    ("s49", (3, 3, 3)),          # pitch 52: the non-generating dropout pass
    ("small", (1, 1, 0)),        # HA 2 < H: sums over the active hops only
    ("small", (3, 0, 0)),        # HA 1
    ("small", (0, 0, 0)),        # HA 0
    ("px0", (3, 3, 3)),          # no mask at all, the switch on: the summed backward on the unmasked map
    ("s900", (3, 3, 3)),         # the fused attention family's bound: tied_bwd.hip's sums over 900 positions
], ids=["small", "edge-h1", "medium-s196", "s49-pitched", "hopw-110", "hopw-300", "hopw-000", "px0", "s900"])
def test_tied_step_against_the_oracle(name, hop_w):
    sh, batch, params, masks = problem(name)
    m = model(sh, params)
    assert m.feature_dropout_tied
    got = step(m, batch, hop_w, masks)
    lay = layouts_of(m)
    m.close()
    assert_close(got, oracle_ref(name, hop_w), lay, f"tied {name} hop_w={hop_w}")
    if not any(hop_w):   # no active hop: nothing runs, the conv gradients are exactly zero
        for lname, sl in util.layer_slices(lay["mult"]):
            if lname.startswith(("i_embed.conv", "attbycontent.ifeatproj")):
                assert not np.any(got["g_mult"][sl]), lname


def test_context_of_8_run_at_5_samples():
    sh, batch, params, masks = problem("b5")
    m = model(sh, params, cap=8)
    m.set_batch_size(5)
    assert m.feature_dropout_tied and m.get_mask("x").shape == (5, sh.D, sh.S)
    got = step(m, batch, (3, 3, 3), masks)
    lay = layouts_of(m)
    m.close()
    assert_close(got, oracle_ref("b5", (3, 3, 3)), lay, "tied, capacity 8 at 5 samples")


def test_image_table_with_repeated_images_in_train_mode():
    sh, batch, params, masks = problem("small")
    image_of = np.array([0, 1, 1, 2, 0, 3, 3, 3], np.int32)
    table = np.ascontiguousarray(batch["feats"][:4])
    plain = dict(batch, feats=np.ascontiguousarray(table[image_of]))
    ref = oracle.step(sh, params, plain["feats"], batch["tokens"], batch["lens"], batch["labels"],
                      replicated(sh, masks), f32((3, 3, 3)), dtype=np.float64)
    m = model(sh, params)
    got = step(m, dict(batch, feats=table, image_of=image_of), (3, 3, 3), masks)
    lay = layouts_of(m)
    m.close()
    assert_close(got, ref, lay, "tied image table")


# ------------------------------------------------------------------ against the per-hop device path
def _both_kinds(batch_kw, loss, what):
    sh, batch, params, masks = problem("small")
    res = []
    for tied in (False, True):
        m = model(sh, params, tied=tied)
        res.append(step(m, dict(batch, **batch_kw), (3, 1, 2), masks if tied else replicated(sh, masks), **loss))
        lay = layouts_of(m)
        m.close()
    assert_close(res[1], res[0], lay, what)


def test_region_counts_against_the_per_hop_path():
    sh = problem("small")[0]
    counts = np.array([12, 1, 5, 7, 12, 3, 9, 2], np.int32)
    assert counts.shape == (sh.B,) and counts.max() <= sh.S
    _both_kinds(dict(regions=counts), {}, "tied with region counts")


def test_select_attention_and_merged_terms_against_the_per_hop_path():
    sh = problem("small")[0]
    t = np.random.default_rng(4).random((sh.B, sh.S)).astype(np.float32)
    t[3] = 0.0   # an unsupervised row
    _both_kinds(dict(att_targets=t), dict(select_w=f32([0.5, 1.0, 0.25]), att_w=f32([0.3, 0.0, 0.7]),
                                          merge_w=f32([0.7, 1.3])), "tied with select / att / merge terms")


def test_module_level_clones_read_the_one_mask():
    """The module-level calls get no tied entry point, but with the switch on their clones must read the ONE mask
    (seeded, or the caller's [B, D, S]) and not a per-hop slice behind it: feval over the module-level calls
    (every clone on its own, nothing summed) gives the tied step's gradients, at the project's TOL."""
    import torch
    from rau_vqa_amd import modules
    sh, batch, params, masks = problem("small")
    hop_w = f32((3, 1, 2))

    def cuda(a, dt=None):
        t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
        return t if dt is None else t.to(dt)
    for explicit in (False, True):
        m = model(sh, params)
        m.set_dropout_seed(77, 5)
        if explicit:
            m.set_masks(masks)
        m.zero_grads()
        modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32), cuda(batch["lens"], torch.int32),
                      cuda(batch["labels"], torch.int32), hop_w)
        m.sync()
        g_mod = m.get_grads()
        g_step = step(m, batch, hop_w)
        m.close()
        for k in g_mod:
            e = util.rel_err(g_mod[k], g_step["g_" + k])
            print(f"module-level vs tied step, {'explicit' if explicit else 'seeded'} masks, {k}: {e:.2e}")
            assert np.max(np.abs(g_mod[k])) > 0 and e < TOL, k


# ------------------------------------------------------------------ element types
@pytest.mark.parametrize("seeded", [False, True], ids=["explicit", "seeded"])
def test_fp16_batch_is_the_f32_batch_of_its_widened_values(seeded):
    sh, batch, params, masks = problem("small")
    half = batch["feats"].astype(np.float16)
    res = []
    for feats in (half, half.astype(np.float32)):
        m = model(sh, params)
        if seeded:
            m.set_dropout_seed(5, 2)
        res.append(step(m, dict(batch, feats=feats), (3, 3, 3), None if seeded else masks))
        m.close()
    assert_same_bits(res[0], res[1], "fp16 vs widened f32 batch, tied")


# ------------------------------------------------------------------ device-drawn masks
def test_seeded_tied_mask_is_hop_0_of_the_per_hop_mask_and_feeds_back_bit_for_bit():
    sh, batch, params, _ = problem("small")
    a = model(sh, params)
    a.set_dropout_seed(9, 4)
    drawn = a.get_mask("x")
    assert drawn.shape == (sh.B, sh.D, sh.S)
    per_hop = model(sh, params, tied=False)
    per_hop.set_dropout_seed(9, 4)
    full = per_hop.get_mask("x")
    per_hop.close()
    assert full.shape == (sh.H, sh.B, sh.D, sh.S)
    assert np.array_equal(drawn, full[0])
    assert 0.3 < drawn.mean() < 0.7 and not np.array_equal(full[0], full[1])
    seeded = step(a, batch, (3, 3, 3))
    a.set_dropout_seed(9, 4)
    a.set_masks({"x": drawn})            # the other four sites stay on the seeded stream
    fed = step(a, batch, (3, 3, 3))
    a.set_dropout_seed(9, 4)
    a.set_masks({"x": drawn[None]})      # [1, B, D, S] is the same mask
    fed1 = step(a, batch, (3, 3, 3))
    a.close()
    assert_same_bits(seeded, fed, "drawn mask fed back")
    assert_same_bits(seeded, fed1, "drawn mask fed back as [1, B, D, S]")


# ------------------------------------------------------------------ determinism and capture
def test_two_tied_steps_give_the_same_bits():
    sh, batch, params, masks = problem("small")
    m = model(sh, params)
    first = step(m, batch, (3, 1, 2), masks)
    second = step(m, batch, (3, 1, 2), masks)
    m.close()
    assert_same_bits(first, second, "repeated tied step")


@pytest.mark.parametrize("name", ["small", "medium"])
def test_graph_step_equals_forward_plus_backward(name):
    sh, batch, params, _ = problem(name)
    hop_w = (2.0,) * sh.H
    eager, graph = model(sh, params), model(sh, params)
    for it in range(2):
        res = []
        for m, use_graph in ((eager, False), (graph, True)):
            m.set_dropout_seed(11, it)
            res.append(step(m, batch, hop_w, graph=use_graph))
        assert_same_bits(res[0], res[1], f"tied graph step {it}")
    eager.close()
    graph.close()


def test_per_hop_graph_survives_a_switch_to_tied_and_back():
    sh, batch, params, _ = problem("small")
    m = model(sh, params, tied=False)
    ref_m = model(sh, params, tied=False)
    m.set_dropout_seed(3, 1)
    ref_m.set_dropout_seed(3, 1)
    want = step(ref_m, batch, (3, 3, 3))
    ref_m.close()
    before = step(m, batch, (3, 3, 3), graph=True)
    m.tie_feature_dropout()
    tied_graph = step(m, batch, (3, 3, 3), graph=True)
    m.tie_feature_dropout(False)
    assert not m.feature_dropout_tied
    after = step(m, batch, (3, 3, 3), graph=True)
    eager_tied = model(sh, params)
    eager_tied.set_dropout_seed(3, 1)
    want_tied = step(eager_tied, batch, (3, 3, 3))
    eager_tied.close()
    m.close()
    assert_same_bits(before, want, "per-hop graph")
    assert_same_bits(after, want, "per-hop graph replayed after tied and back")
    assert_same_bits(tied_graph, want_tied, "tied graph captured in between")
    assert not np.array_equal(tied_graph["g_mult"], want["g_mult"])


# ------------------------------------------------------------------ switch semantics
def test_default_is_per_hop_and_the_switch_off_changes_no_bit():
    sh, batch, params, masks = problem("small")
    plain = model(sh, params, tied=False)
    assert not plain.feature_dropout_tied
    want = step(plain, batch, (3, 3, 3), replicated(sh, masks))
    plain.close()
    m = model(sh, params, tied=False)
    m.tie_feature_dropout()
    m.tie_feature_dropout(False)
    got = step(m, batch, (3, 3, 3), replicated(sh, masks))
    m.close()
    assert_same_bits(got, want, "switched on and off again")


def test_switch_between_forward_and_backward_and_bad_arguments():
    from rau_vqa_amd import _lib
    sh, batch, params, masks = problem("small")
    m = model(sh, params, tied=False)
    lib = _lib.lib()
    assert lib.rau_set_feat_dropout(m._h, 2) == -1 and lib.rau_set_feat_dropout(m._h, -1) == -1   # RAU_ERR_INVALID
    assert not m.feature_dropout_tied
    m.set_masks(replicated(sh, masks))
    m.set_batch(**batch)
    m.zero_grads()
    m.forward()
    m.tie_feature_dropout()
    with pytest.raises(_lib.RauError, match="librau error -3"):   # RAU_ERR_STATE
        m.backward(f32((3, 3, 3)))
    # the per-hop mask does not fit the tied site: refused by the host layer and by the library
    full = replicated(sh, masks)["x"]
    with pytest.raises(ValueError):
        m.set_masks({"x": full})
    assert lib.rau_set_mask(m._h, _lib.MASK_SITES["x"], full.ctypes.data, full.size) == -1
    # the change dropped the caller's x mask: the site is back on the seeded stream, the step runs
    m.set_masks({k: v for k, v in masks.items() if k != "x"})
    m.set_masks({"x": masks["x"]})
    got = step(m, batch, (3, 3, 3))
    lay = layouts_of(m)
    m.close()
    assert_close(got, oracle_ref("small", (3, 3, 3)), lay, "tied after a refused mask")


# ------------------------------------------------------------------ launch counts: the saving is structural
def _profiled_step(sh, batch, params, masks, tied):
    m = model(sh, params, tied=tied)
    m.set_masks(masks)
    m.set_batch(**batch)
    m.zero_grads()
    m.prof_enable(True)
    m.forward()
    m.backward(f32((3, 3, 3)))
    m.sync()
    prof = m.prof()
    m.prof_enable(False)
    m.close()
    return prof


def test_a_tied_step_launches_every_conv_once():
    """SMALL at H = 3.  Tied: each of the five conv classes once over forward + backward, hop_sum and outer_sum
    once.  Per-hop, the same step: H times the conv FLOPs of each class.  Its launch count depends on the hop-group
    partition, which at up to 64 samples is ONE group of H hops (one launch of 3B samples), so "more than one
    conv_att_dgrad launch per-hop" is asserted on the same widths at B = 72, where the default partition is 1, 1, 1."""
    sh, batch, params, masks = problem("small")
    tied = _profiled_step(sh, batch, params, masks, True)
    for cls in CONVS + ("hop_sum", "outer_sum"):
        assert tied[cls]["launches"] == 1, (cls, tied.get(cls))
    per_hop = _profiled_step(sh, batch, params, replicated(sh, masks), False)
    assert "hop_sum" not in per_hop and "outer_sum" not in per_hop
    for cls in CONVS:
        assert per_hop[cls]["flops"] == sh.H * tied[cls]["flops"], cls
    sh72 = util.shapes(dict(util.SMALL, B=72))
    batch72, params72, masks72 = util.make_problem(sh72, scale=0.5)
    wide = _profiled_step(sh72, batch72, params72, masks72, False)
    assert wide["conv_att_dgrad"]["launches"] > 1, wide["conv_att_dgrad"]
    wide_tied = _profiled_step(sh72, batch72, params72, dict(masks72, x=np.ascontiguousarray(masks72["x"][0])), True)
    for cls in CONVS + ("hop_sum", "outer_sum"):
        assert wide_tied[cls]["launches"] == 1, (cls, wide_tied.get(cls))


# ------------------------------------------------------------------ bf16 mode: bar (2) of tests/test_gpu_bf16.py
@pytest.mark.parametrize("name", ["small", "medium"])
def test_bf16_tied_step_against_the_exact_oracle(name):
    """The tied backward rounds dS and dZ once, as sums over the hops: fewer roundings than the emulation's one per
    hop, so only the exact-oracle bar applies: outputs within TOL_EXACT of their max norm, gradients within
    TOL_EXACT_GRAD of the un-cancelled magnitude max(max |g|, max sum_b |g_b|)."""
    from oracle import ref_torch as RT
    from tests.test_gpu_bf16 import TOL_EXACT, TOL_EXACT_GRAD
    sh, batch, params, masks = problem(name)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    exact = RT.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"],
                    replicated(sh, masks), hop_w, per_sample_abs=True)
    m = model(sh, params, dtype="bf16")
    got = step(m, batch, hop_w, masks)
    lay = layouts_of(m)
    m.close()
    bad, worst = {}, (0.0, 0.0)
    for k in util.OUT_KEYS:
        e = util.rel_err(got[k], np.asarray(exact[k]))
        worst = (max(worst[0], e / TOL_EXACT), worst[1])
        if not e < TOL_EXACT:
            bad[k] = (e, TOL_EXACT)
    for grp in lay:
        for lname, sl in util.layer_slices(lay[grp]):
            ref = np.asarray(exact["g_" + grp])[sl]
            scale = max(float(np.max(np.abs(ref))), float(np.max(np.asarray(exact["gabs_" + grp])[sl])))
            e = float(np.max(np.abs(got["g_" + grp][sl] - ref)))
            e = e / scale if scale > 1e-12 else e
            worst = (worst[0], max(worst[1], e / TOL_EXACT_GRAD))
            if not e < TOL_EXACT_GRAD:
                bad[lname] = (e, TOL_EXACT_GRAD)
    print(f"bf16 tied {name}: largest error / bar: outputs {worst[0]:.3f}, gradients {worst[1]:.3f}")
    assert not bad, f"vs exact oracle, (error, bar): {bad}"
