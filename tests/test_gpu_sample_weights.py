"""Per-sample loss weights on the GPU (rau_set_sample_weights, rau_get_loss_rows, rau_dev_scale_rows): every built-in
mean (1/n) sum_b row_b of the step path becomes (1/n) sum_b s_b row_b.

The fp64 reference is the unchanged tests/ext_ref.py, called on the batch with labels=None and hop_w=None and given the
WHOLE weighted objective as its callable F (weighted_objective below): hop_w CE_h, select_w BCE_h, att_w ATT_h and the
two merged rows, each as the weighted mean of its per-sample rows.  The machinery is tests/test_gpu_select.py's,
tests/test_gpu_merged.py's and tests/test_gpu_ext.py's: the committed problems under their explicit masks, make_model,
grad_errs, same_bits, TOL = 1e-4 per layer slice, and in bf16 mode the bar tests/test_gpu_bf16.py derives.

Weights: uniform in [0, 2] with one exact zero (sample ZERO).  With them the oracle's gradients differ from the
unweighted ones by more than 0.3 relative in every parameter group (asserted once below; measured 0.39 / 0.48 / 0.80 for
embed / rnn / mult under HOP_W), so a build that ignores the weights fails every parity case.
"""
import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from rau_vqa_amd import joint, predict
from tests import att_ref, bce_ref, ext_ref, merge_ref, util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_ext import COUNTS8
from tests.test_gpu_merged import step as merged_step
from tests.test_gpu_select import (GROUPS, INVALID, STATE, TOL, check_argmax, f32, grad_errs, make_model, problem,
                                   same_bits, small_answer_set, targets)

pytestmark = pytest.mark.gpu

ZERO = 3                                   # the sample whose weight is exactly 0
EPS = 1e-12
HOP_W, SELECT_W, ATT_W, MERGE_W = [3, 0.5, 2], [0.7, 0.4, 1.3], [0.5, 3.0, 1.5], [0.7, 1.3]


# ------------------------------------------------------------------------------------------ machinery
def weights(n, seed=1):
    s = np.random.default_rng(seed).uniform(0, 2, size=n).astype(np.float32)
    s[ZERO] = 0.0
    return s


def weighted_objective(sh, batch, s, hop_w, answers=None, loss="ce", select_w=None, t_gt=None, att_w=None, att_t=None,
                       nreg=None, merge_w=None, keep=None):
    """F for ext_ref.step: sum_h hop_w[h] WM(CE rows_h) + select_w[h] WM(BCE rows_h) + att_w[h] WM(ATT rows_h)
    + merge_w[0] WM(CE rows(uni)) + merge_w[1] WM(CE rows(select)), WM(rows) = (1/n) sum_b s_b rows_b.  The criterion
    rows are ext_ref.step's own statements without their mean.  keep["rows"]: the weighted criterion rows per hop."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    sv, B = t(s), sh.B
    if loss == "bce":
        tgt, lab = bce_ref.target(sh, batch, answers)
        tgt, live = t(tgt), t(lab.astype(np.float64)).unsqueeze(1)
        rows = lambda sc: (torch.nn.functional.binary_cross_entropy_with_logits(sc, tgt, reduction="none") * live).sum(1)
    elif answers is not None:
        ids = torch.as_tensor(answers[0]).long()
        aw = torch.where(ids > 0, t(answers[1]), torch.zeros((), dtype=torch.float64))
        rows = lambda sc: (aw * (torch.logsumexp(sc, dim=1, keepdim=True)
                                 - torch.gather(sc, 1, (ids - 1).clamp(min=0)))).sum(1)
    else:
        y = torch.as_tensor(batch["labels"]).long() - 1
        rows = lambda sc: torch.nn.functional.cross_entropy(sc, y, reduction="none")
    wm = lambda r: (sv * r).sum() / B

    def F(scores, dps, atts):
        total = 0.0
        for h in range(sh.H):
            r = rows(scores[h])
            if keep is not None:
                keep.setdefault("rows", []).append((sv * r).detach().numpy())
            total = total + float(hop_w[h]) * wm(r)
            if select_w is not None:
                tg, dp = t(t_gt[h]), dps[h]
                total = total + float(select_w[h]) * wm(-(tg * torch.log(dp + EPS) + (1 - tg) * torch.log(1 - dp + EPS)))
            if att_w is not None:
                tb = t(att_t)
                if nreg is not None:
                    tb = tb * (torch.arange(sh.S)[None, :] < torch.as_tensor(np.asarray(nreg))[:, None])
                total = total + float(att_w[h]) * wm((tb * -torch.log(atts[h] + EPS)).sum(1))
        if merge_w is not None:
            gate = t(merge_ref.first_fire(np.stack([d.detach().numpy() for d in dps])))      # a constant
            uni = torch.stack(scores).mean(dim=0)
            select = sum(scores[h] * gate[h].unsqueeze(1) for h in range(sh.H))
            total = total + float(merge_w[0]) * wm(rows(uni)) + float(merge_w[1]) * wm(rows(select))
        return total
    return F


def reference(sh, params, batch, masks, s, hop_w, bf16=False, **terms):
    """ext_ref.step on the batch WITHOUT labels and hop weights, the weighted objective as F; also the weighted
    criterion rows [H, n] of that forward."""
    keep = {}
    F = weighted_objective(sh, batch, s, hop_w, keep=keep, **terms)
    ref = ext_ref.step(sh, params, dict(batch, labels=None), masks, None, F=F, nreg=terms.get("nreg"), bf16=bf16)
    ref["rows"] = np.stack(keep["rows"][:sh.H])
    return ref


def dev_step(m, hop_w, select_w=None, att_w=None, merge_w=None, how="merged"):
    """zero_grads + forward + backward through rau_backward_merged (None = NULL: the plain rau_backward) or, how =
    "graph", rau_graph_step_merged."""
    return merged_step(m, hop_w, merge_w, select_w, att_w, how=how)


def put(m, batch, **kw):
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], **kw)


def assert_within(got, ref, layouts, what, tol=TOL):
    errs = grad_errs(got, ref, layouts)
    worst = max(errs, key=errs.get)
    print(f"{what}: largest error {errs[worst]:.1e} ({worst})")
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, f"{what}: relative errors above {tol}: {bad}"


def check_rows(m, ref, s, what):
    """rau_get_loss_rows and rau_get_losses against the oracle's weighted rows; the zero-weight row is exactly 0."""
    rows, losses = m.loss_rows(), m.losses()
    assert rows.shape == ref["rows"].shape and rows.dtype == np.float32
    print(f"{what}: rows {util.rel_err(rows, ref['rows']):.1e} losses {util.rel_err(losses, ref['rows'].mean(1)):.1e}")
    assert util.rel_err(rows, ref["rows"]) < TOL and util.rel_err(losses, ref["rows"].mean(1)) < TOL
    assert np.all(rows[:, s == 0] == 0)
    assert util.rel_err(losses, joint.weighted_mean(rows)) < 1e-6     # the losses are the means of these rows
    return rows, losses


def gates_agree(m, fwd):
    """The condition of every case with a select_w or merge_w: the device's gates and answers are the oracle's."""
    assert np.abs(fwd["dopred"] - 0.5).min() > 1e-4, "a do_pred of the oracle within 1e-4 of the gate: another seed"
    assert np.array_equal(m.dopred() > 0.5, fwd["dopred"] > 0.5)
    return targets(check_argmax(m, fwd), {"labels": fwd["labels"]})


def forward_ref(sh, params, batch, masks, nreg=None):
    fwd = ext_ref.step(sh, params, batch, masks, [0.0] * sh.H, backward=False, nreg=nreg)
    fwd["labels"] = batch["labels"]
    return fwd


def small_with_att(counts):
    sh, batch, params, masks = problem("SMALL")
    nreg = COUNTS8 if counts else None
    fwd = forward_ref(sh, params, batch, masks, nreg)
    t = att_ref.targets(fwd["att"], nreg)
    assert att_ref.check(fwd["att"], t, nreg)
    return sh, batch, params, masks, nreg, fwd, t


# ------------------------------------------------------------------------------------------ 1. parity at SMALL
@pytest.mark.parametrize("evaluate", [False, True], ids=["train", "evaluate"])
@pytest.mark.parametrize("target", ["labels", "set", "bce_labels", "bce_set"])
def test_criterion_parity(target, evaluate):
    sh, batch, params, masks = problem("SMALL")
    s = weights(sh.B)
    answers = small_answer_set(batch, sh) if target.endswith("set") else None
    loss = "bce" if target.startswith("bce") else "ce"
    masks = None if evaluate else masks
    m = make_model(sh, params, masks)
    if evaluate:
        m.evaluate()
    m.set_answer_loss(loss)
    put(m, batch, sample_w=s, **({} if answers is None else {"answers": answers}))
    assert m.batch_sample_weights
    got = dev_step(m, HOP_W)
    layouts = {k: m.layout(k) for k in GROUPS}
    ref = reference(sh, params, batch, masks, s, HOP_W, answers=answers, loss=loss)
    check_rows(m, ref, s, f"{target} {'evaluate' if evaluate else 'train'}")
    m.close()
    assert_within(got, ref, layouts, target)
    if target == "labels" and not evaluate:      # the weights are at work in the oracle: ignoring them cannot pass
        plain = ext_ref.step(sh, params, batch, masks, HOP_W)
        diff = [util.rel_err(ref["g_" + k], plain["g_" + k]) for k in GROUPS]
        print("weighted vs unweighted oracle:", diff)
        assert min(diff) > 0.3


def test_bf16_mode_against_the_emulated_oracle():
    sh, batch, params, masks = problem("SMALL")
    s = weights(sh.B)
    m = make_model(sh, params, masks, dtype="bf16")
    put(m, batch, sample_w=s)
    got = dev_step(m, HOP_W)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    with RT.bf16_emulation():
        emu = reference(sh, params, batch, masks, s, HOP_W, bf16=True)
    nudged = []
    for n in NUDGES:
        with RT.bf16_emulation(n):
            nudged.append(reference(sh, params, batch, masks, s, HOP_W, bf16=True))
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
    print(f"bf16 weights: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated oracle, (error, derived bar): {bad}"


# ------------------------------------------------------------------------------------------ 2. all terms together
_ALL = {}


def all_terms_reference():
    """SMALL, every term, targets but no counts: the oracle, computed once (cases 2's twin without counts, 7)."""
    if not _ALL:
        sh, batch, params, masks, _n, fwd, t = small_with_att(False)
        _ALL.update(fwd=fwd, t=t, s=weights(sh.B))
    return _ALL


def test_all_terms_with_counts_eager_and_captured():
    sh, batch, params, masks, nreg, fwd, t = small_with_att(True)
    s = weights(sh.B)
    m = make_model(sh, params, masks)
    put(m, batch, regions=nreg, att_targets=t, sample_w=s)
    got = dev_step(m, HOP_W, SELECT_W, ATT_W, MERGE_W)
    t_gt = gates_agree(m, fwd)
    rows = m.loss_rows()
    layouts = {k: m.layout(k) for k in GROUPS}
    graph = dev_step(m, HOP_W, SELECT_W, ATT_W, MERGE_W, how="graph")
    same_bits(graph, got)
    assert np.array_equal(m.loss_rows(), rows)
    same_bits(dev_step(m, HOP_W, SELECT_W, ATT_W, MERGE_W, how="graph"), got)      # the replay
    m.close()
    ref = reference(sh, params, batch, masks, s, HOP_W, select_w=SELECT_W, t_gt=t_gt, att_w=ATT_W, att_t=t, nreg=nreg,
                    merge_w=MERGE_W)
    assert util.rel_err(rows, ref["rows"]) < TOL
    assert_within(got, ref, layouts, "all terms with counts")


# ------------------------------------------------------------------------------------------ 3. kernel classes
def class_parity(sh, batch, params, masks, hop_w, select_w=None, merge_w=None, what=""):
    s = weights(sh.B)
    fwd = forward_ref(sh, params, batch, masks)
    m = make_model(sh, params, masks)
    put(m, batch, sample_w=s)
    got = dev_step(m, hop_w, select_w, None, merge_w)
    t_gt = gates_agree(m, fwd) if (select_w is not None or merge_w is not None) else None
    layouts = {k: m.layout(k) for k in GROUPS}
    ref = reference(sh, params, batch, masks, s, hop_w, select_w=select_w, t_gt=t_gt, merge_w=merge_w)
    check_rows(m, ref, s, what)
    m.close()
    assert_within(got, ref, layouts, what)


def test_edge_shape():
    sh, batch, params, masks = problem("EDGE")
    class_parity(sh, batch, params, masks, [1], [0.9], MERGE_W, "EDGE")


def test_pitched_logits_rows_K13():
    sh = util.shapes(util.SMALL, K=13)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    class_parity(sh, batch, params, masks, HOP_W, SELECT_W, MERGE_W, "K = 13")


def test_medium_shape_partials_finished_inside_the_head():
    sh, batch, params, masks = problem("MEDIUM")
    class_parity(sh, batch, params, masks, [2, 2], what="MEDIUM")


def test_unstaged_merge_grad_K4100():
    sh = util.shapes(util.SMALL, K=4100)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    class_parity(sh, batch, params, masks, HOP_W, None, MERGE_W, "K = 4100")


# ------------------------------------------------------------------------------------------ 4. bit for bit
def full_step(m, how="merged"):
    return dev_step(m, HOP_W, SELECT_W, ATT_W, MERGE_W, how=how)


def test_weights_all_one_are_no_weights_bit_for_bit_and_launch_for_launch():
    a = all_terms_reference()
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    m.prof_enable()

    def run():
        m.prof_reset()
        g = full_step(m)
        m.sync()
        listing = {n: v["launches"] for n, v in m.prof().items() if v["launches"]}
        return g, listing, m.logits(), m.dopred(), m.losses(), m.loss_rows(), m.step_stats(), m.att_stats()

    put(m, batch, att_targets=a["t"])
    assert not m.batch_sample_weights
    base = run()
    m.set_sample_weights(np.ones(sh.B, np.float32))
    assert m.batch_sample_weights
    ones = run()
    same_bits(ones[0], base[0])
    assert ones[1] == base[1] and ones[1]["merge_grad"] == 1 and ones[1]["select_signal"] == 1
    for x, y in zip(ones[2:6], base[2:6]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for x, y in zip(ones[6:], base[6:]):
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    m.set_sample_weights(a["s"])                      # and real weights change the numbers, not the launches
    real = run()
    assert real[1] == base[1]
    assert all(not np.array_equal(real[0][k], base[0][k]) for k in GROUPS)
    m.close()


def test_detaching_restores_the_unweighted_step_and_both_captured_steps_coexist():
    a = all_terms_reference()
    sh, batch, params, masks = problem("SMALL")
    s, s2 = a["s"], weights(sh.B, seed=2)
    m = make_model(sh, params, masks)
    put(m, batch, att_targets=a["t"])
    plain = full_step(m)
    same_bits(full_step(m, "graph"), plain)              # captured without weights
    m.set_sample_weights(s)
    eager = full_step(m)
    assert any(not np.array_equal(eager[k], plain[k]) for k in GROUPS)
    same_bits(full_step(m, "graph"), eager)              # captured with weights: another graph
    m.clear_sample_weights()
    assert not m.batch_sample_weights
    same_bits(full_step(m, "graph"), plain)              # the unweighted graph again
    same_bits(full_step(m), plain)
    m.set_sample_weights(s2)                             # a replay reads the CURRENT weights
    got2 = full_step(m, "graph")
    same_bits(full_step(m), got2)
    assert any(not np.array_equal(got2[k], eager[k]) for k in GROUPS)
    m.set_sample_weights(s)
    same_bits(full_step(m, "graph"), eager)
    assert m._lib.rau_set_sample_weights(m._h, -1, None) == 0 and m._lib.rau_set_sample_weights(m._h, -1, None) == 0
    m.forward()                                          # the Python forms
    m.set_sample_weights(s, normalize=True)
    with pytest.raises(L.RauError):                      # a forward that ran without them must be run again
        m.backward(f32(HOP_W))
    m.close()


def test_weights_all_two_against_doubled_term_weights():
    """Both are the same arithmetic up to exact power-of-two scalings; only subnormals can differ."""
    a = all_terms_reference()
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    put(m, batch, att_targets=a["t"], sample_w=np.full(sh.B, 2.0, np.float32))
    two = full_step(m)
    rows2 = m.loss_rows()
    layouts = {k: m.layout(k) for k in GROUPS}
    m.clear_sample_weights()
    dbl = dev_step(m, *[[2 * w for w in ws] for ws in (HOP_W, SELECT_W, ATT_W, MERGE_W)])
    assert np.array_equal(rows2, np.float32(2) * m.loss_rows())
    m.close()
    assert_within(two, {"g_" + k: dbl[k] for k in GROUPS}, layouts, "weights 2.0 vs doubled terms", tol=1e-6)


# ------------------------------------------------------------------------------------------ 5. zero rows
def test_a_zero_weight_sample_contributes_nothing_whatever_it_holds():
    """Sample ZERO has weight 0 in both runs; its features, label and attention target differ wildly between them.
    Every gradient is the same: its rows of d_logits, of the select signal, of the attention addend and of the merged
    terms are zero in both."""
    a = all_terms_reference()
    sh, batch, params, masks = problem("SMALL")
    s = a["s"]
    assert s[ZERO] == 0
    wild = {k: np.array(v, copy=True) for k, v in batch.items()}
    wild["feats"][ZERO] = -37.0 * batch["feats"][ZERO] + 5.0
    wild["labels"][ZERO] = batch["labels"][ZERO] % sh.K + 1
    t_wild = a["t"].copy()
    t_wild[ZERO] = t_wild[ZERO][::-1] * 11
    m = make_model(sh, params, masks)
    put(m, batch, att_targets=a["t"], sample_w=s)
    calm = full_step(m)
    rows = m.loss_rows()
    lg = m.logits()
    put(m, wild, att_targets=t_wild, sample_w=s)
    loud = full_step(m)
    rows_w = m.loss_rows()
    assert np.isfinite(m.logits()).all() and not np.array_equal(m.logits()[:, ZERO], lg[:, ZERO])
    for k in GROUPS:
        assert np.isfinite(loud[k]).all() and np.array_equal(loud[k], calm[k]), k
    assert np.all(rows[:, ZERO] == 0) and np.all(rows_w[:, ZERO] == 0)
    assert np.array_equal(np.delete(rows, ZERO, 1), np.delete(rows_w, ZERO, 1))
    st = m.step_stats()
    assert np.isfinite(st["loss"]).all() and np.isfinite(st["loss_do_pred"]).all()
    s1 = s.copy()
    s1[ZERO] = 1.0                                     # with a weight the wild sample is felt
    m.set_sample_weights(s1)
    felt = full_step(m)
    assert any(not np.array_equal(felt[k], calm[k]) for k in GROUPS)
    m.close()


# ------------------------------------------------------------------------------------------ 6. lifetime and errors
def raw_set(m, slot, s):
    return m._lib.rau_set_sample_weights(m._h, slot, None if s is None else f32(s).ctypes.data)


def test_slot_semantics_on_both_upload_paths():
    sh, batch, params, masks = problem("SMALL")
    s = weights(sh.B)
    m = make_model(sh, params, masks)
    assert raw_set(m, -1, s) == STATE and raw_set(m, 0, s) == STATE       # no batch anywhere yet
    assert m._lib.rau_get_loss_rows(m._h, np.empty((sh.H, sh.B), np.float32).ctypes.data) == STATE
    put(m, batch)
    assert m._lib.rau_get_loss_rows(m._h, np.empty((sh.H, sh.B), np.float32).ctypes.data) == STATE   # no forward yet
    plain = dev_step(m, HOP_W)
    m.set_sample_weights(s)
    want = dev_step(m, HOP_W)
    rows = m.loss_rows()
    assert any(not np.array_equal(want[k], plain[k]) for k in GROUPS)
    put(m, batch)                                        # a new upload into the slot clears them
    assert not m.batch_sample_weights
    same_bits(dev_step(m, HOP_W), plain)
    m.set_sample_weights(s)
    m.set_batch_size(5)                                  # ... and so does rau_set_batch_size
    assert raw_set(m, -1, s[:5]) == STATE
    m.set_batch_size(sh.B)
    m.set_masks(masks)
    assert raw_set(m, -1, s) == STATE
    put(m, batch)
    assert not m.batch_sample_weights
    same_bits(dev_step(m, HOP_W), plain)
    # the asynchronous path: between set_batch_async and use_batch, on the copy stream
    assert raw_set(m, 1, s) == STATE                     # slot 1 holds no batch
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.set_sample_weights(s, slot=1)
    assert not m.batch_sample_weights                    # slot 0 is still the resident batch
    m.use_batch(1)
    assert m.batch_sample_weights                        # current together with the batch
    same_bits(dev_step(m, HOP_W), want)
    assert np.array_equal(m.loss_rows(), rows)
    m.set_batch_async(0, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])   # the other slot: left alone
    assert m.batch_sample_weights
    same_bits(dev_step(m, HOP_W), want)
    m.use_batch(0)
    assert not m.batch_sample_weights
    same_bits(dev_step(m, HOP_W), plain)
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], sample_w=s)
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])   # a later upload clears them
    m.use_batch(1)
    assert not m.batch_sample_weights
    same_bits(dev_step(m, HOP_W), plain)
    m.forward()
    assert raw_set(m, 1, s) == STATE                     # the current batch of a forward whose backward has not run
    assert raw_set(m, -1, s) == 0                        # the resident form may: the forward is dropped
    assert raw_set(m, 2, s) == INVALID
    m.close()


def test_invalid_weights_leave_the_previous_ones_in_force():
    sh, batch, params, masks = problem("SMALL")
    s = weights(sh.B)
    m = make_model(sh, params, masks)
    put(m, batch, sample_w=s)
    want = dev_step(m, HOP_W)
    for bad in (np.nan, np.inf, -np.inf, -0.5):
        x = np.ones(sh.B, np.float32)
        x[5] = bad
        assert raw_set(m, -1, x) == INVALID, bad
        assert m.batch_sample_weights
        same_bits(dev_step(m, HOP_W), want)
    m.close()


def test_image_table_and_bank_batches_give_the_plain_batch_bits():
    sh, batch, params, masks = problem("SMALL")
    s = weights(sh.B)
    image_of = np.array([0, 1, 2, 3, 4, 0, 1, 2], np.int32)
    table = np.ascontiguousarray(batch["feats"][:5])
    m = make_model(sh, params, masks)
    m.set_batch(np.ascontiguousarray(table[image_of]), batch["tokens"], batch["lens"], batch["labels"], sample_w=s)
    want = dev_step(m, HOP_W, SELECT_W, None, MERGE_W)
    rows = m.loss_rows()
    m.set_batch(table, batch["tokens"], batch["lens"], batch["labels"], image_of=image_of, sample_w=s)
    assert m.batch_images() == 5 and m.batch_sample_weights
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), want)
    assert np.array_equal(m.loss_rows(), rows)
    m.bank_create(7)
    m.bank_put(1, table)
    m.set_batch(None, batch["tokens"], batch["lens"], batch["labels"], bank_rows=np.arange(1, 6, dtype=np.int32),
                image_of=image_of, sample_w=s)
    assert m.batch_sample_weights
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), want)
    assert np.array_equal(m.loss_rows(), rows)
    m.close()


def test_typed_packed_and_device_batches_with_an_attached_question_give_the_plain_batch_bits():
    """The weights are per SAMPLE whatever form the batch takes: a 16-bit batch, packed region rows, maps taken from
    device memory (rau_set_batch_dev), and a question attached behind the upload."""
    from rau_vqa_amd import feat16
    sh, batch, params, masks = problem("SMALL")
    s = weights(sh.B)
    half = batch["feats"].astype(np.float16)                       # values a 16-bit batch holds exactly
    wide = dict(batch, feats=half.astype(np.float32))
    m = make_model(sh, params, masks)
    put(m, wide)
    plain = dev_step(m, HOP_W, SELECT_W, None, MERGE_W)
    put(m, wide, sample_w=s)
    want = dev_step(m, HOP_W, SELECT_W, None, MERGE_W)
    rows = m.loss_rows()
    assert any(not np.array_equal(want[k], plain[k]) for k in GROUPS)
    # a typed batch
    m.set_batch(half, batch["tokens"], batch["lens"], batch["labels"], sample_w=s)
    assert m.batch_feat_type() == "f16" and m.batch_sample_weights
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), want)
    assert np.array_equal(m.loss_rows(), rows)
    # maps from device memory
    x = torch.as_tensor(wide["feats"]).cuda()
    torch.cuda.synchronize()
    m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"], sample_w=s)
    assert m.batch_sample_weights
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), want)
    m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"])          # a later upload clears them
    assert not m.batch_sample_weights
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), plain)
    # ... with a question attached behind the upload
    q = torch.as_tensor(np.random.default_rng(8).normal(size=(sh.B, 4 * sh.Rq)).astype(np.float32) * 0.5).cuda()
    torch.cuda.synchronize()
    put(m, wide)
    m.set_question(q)
    q_plain = dev_step(m, HOP_W, SELECT_W, None, MERGE_W)
    put(m, wide, sample_w=s)
    m.set_question(q)
    assert m.batch_question and m.batch_sample_weights
    q_want = dev_step(m, HOP_W, SELECT_W, None, MERGE_W)
    q_rows = m.loss_rows()
    assert any(not np.array_equal(q_want[k], q_plain[k]) for k in GROUPS)
    assert any(not np.array_equal(q_want[k], want[k]) for k in GROUPS)
    assert np.all(q_rows[:, ZERO] == 0)
    m.set_batch_dev(x, batch["tokens"], batch["lens"], batch["labels"], question=q, sample_w=s)
    assert m.batch_question and m.batch_sample_weights
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), q_want)
    assert np.array_equal(m.loss_rows(), q_rows)
    m.clear_sample_weights()                                        # the question stays, the weights go
    assert m.batch_question and not m.batch_sample_weights
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), q_plain)
    # packed region rows: the batch brings its counts, the weights are attached to it like to any other
    packed = np.concatenate([wide["feats"][b][:, :n].T for b, n in enumerate(COUNTS8)]).astype(np.float32)
    dense = feat16.unpack_regions(packed, COUNTS8, sh.S)
    m.set_batch(dense, batch["tokens"], batch["lens"], batch["labels"], regions=COUNTS8, sample_w=s)
    p_want = dev_step(m, HOP_W, SELECT_W, None, MERGE_W)
    m.set_batch_packed(packed, COUNTS8, batch["tokens"], batch["lens"], batch["labels"])
    assert m.batch_regions() and not m.batch_sample_weights
    m.set_sample_weights(s)
    same_bits(dev_step(m, HOP_W, SELECT_W, None, MERGE_W), p_want)
    m.close()
    del x, q


# ------------------------------------------------------------------------------------------ 7. rau_dev_scale_rows
@pytest.mark.parametrize("cols", [1, 4, 13, 1000])
def test_dev_scale_rows_against_numpy(cols):
    sh, _batch, params, _masks = problem("EDGE")
    m = make_model(sh, params)
    rows = 37
    rng = np.random.default_rng(cols)
    s = rng.uniform(0, 2, size=rows).astype(np.float32)
    s[ZERO] = 0
    for ld in sorted({cols, (cols + 3) // 4 * 4}):
        for off in (0, 1):                         # off 1: a base that is not 16-byte aligned (scalar accesses)
            x = rng.normal(size=rows * ld + off).astype(np.float32)
            xd = torch.as_tensor(x).cuda()
            sd = torch.as_tensor(s).cuda()
            torch.cuda.synchronize()
            L.check(m._lib.rau_dev_scale_rows(m._h, xd.data_ptr() + 4 * off, rows, cols, ld, sd.data_ptr()))
            m.sync()
            got = xd.cpu().numpy()
            want = x.copy()
            body = want[off:].reshape(rows, ld)
            body[:, :cols] = body[:, :cols] * s[:, None]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cols, ld, off)
    assert m._lib.rau_dev_scale_rows(m._h, xd.data_ptr(), rows, cols, cols - 1, sd.data_ptr()) == INVALID
    m.close()


def test_module_level_feval_with_sample_weights_against_the_step_path():
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda
    a = all_terms_reference()
    sh, batch, params, masks = problem("SMALL")
    s, t = a["s"], a["t"]
    m = make_model(sh, params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.zero_grads()
    modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32), cuda(batch["lens"], torch.int32),
                  cuda(batch["labels"], torch.int32), HOP_W, select_w=SELECT_W, att_w=ATT_W, att_targets=cuda(t),
                  merge_w=MERGE_W, sample_w=cuda(s))
    m.sync()
    g_mod = m.get_grads()
    put(m, batch, att_targets=t, sample_w=s)
    g_step = full_step(m)
    t_gt = gates_agree(m, a["fwd"])
    m.close()
    ref = reference(sh, params, batch, masks, s, HOP_W, select_w=SELECT_W, t_gt=t_gt, att_w=ATT_W, att_t=t,
                    merge_w=MERGE_W)
    assert_within(g_mod, ref, layouts, "feval(sample_w=) vs the oracle")
    assert_within(g_step, ref, layouts, "step path vs the oracle")
    # the two device paths against each other, on the oracle's scale per layer (tests/test_gpu_att_targets.py's rule)
    errs = {}
    for grp in GROUPS:
        for name, sl in util.layer_slices(layouts[grp]):
            den = np.max(np.abs(ref["g_" + grp][sl]))
            errs[name] = float(np.max(np.abs(g_step[grp][sl] - g_mod[grp][sl])) / (den if den >= 1e-12 else 1.0))
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"step level vs feval above {TOL}: {bad}"


# ------------------------------------------------------------------------------------------ 8. statistics
@pytest.mark.parametrize("target", ["labels", "set", "bce_set"])
def test_statistics_take_the_weight_per_row_and_counts_do_not(target):
    a = all_terms_reference()
    sh, batch, params, masks = problem("SMALL")
    s, t = a["s"], a["t"]
    answers = small_answer_set(batch, sh) if target.endswith("set") else None
    loss = "bce" if target.startswith("bce") else "ce"
    m = make_model(sh, params, masks)
    m.set_answer_loss(loss)
    kw = {} if answers is None else {"answers": answers}
    put(m, batch, att_targets=t, regions=COUNTS8, **kw)
    m.forward()
    plain, plain_att, plain_pred = m.step_stats(), m.att_stats(), m.predict()[0]
    scores = m.step_scores() if answers is not None else None
    put(m, batch, att_targets=t, regions=COUNTS8, sample_w=s, **kw)
    m.forward()
    got, got_att = m.step_stats(), m.att_stats()
    logits, dopred, att = m.logits(), m.dopred(), m.attention()
    assert np.array_equal(got["loss"][:sh.H], m.losses())                     # bitwise rau_get_losses
    assert util.rel_err(m.losses(), joint.weighted_mean(m.loss_rows())) < 1e-6
    if answers is None:
        want = joint.feval_stats(logits, dopred, batch["labels"], sample_w=s)
    else:
        want = predict.set_stats(logits, dopred, *answers, loss=loss, sample_w=s)
        again = m.step_scores()
        assert np.array_equal(again[0], scores[0]) and np.array_equal(again[1], scores[1])   # the metric: unweighted
    print("loss", got["loss"], want["loss"], "do_pred", got["loss_do_pred"], want["loss_do_pred"])
    assert util.rel_err(got["loss"], want["loss"]) < 1e-4
    assert util.rel_err(got["loss_do_pred"], want["loss_do_pred"]) < 1e-4
    assert util.rel_err(got["loss"], plain["loss"]) > 1e-2                    # the weights are at work
    for k in ("correct", "do_pred_correct", "did_correct", "fired", "selected"):
        assert np.array_equal(got[k], plain[k]), k                            # counts: unchanged
    want_att = joint.att_stats(att, t, COUNTS8, sample_w=s)
    assert np.all(np.abs(got_att["loss"] - want_att["loss"]) <= 1e-5 * np.abs(want_att["loss"]))
    assert not np.array_equal(got_att["loss"], plain_att["loss"])
    for k in ("mass", "hits"):
        assert np.array_equal(got_att[k], plain_att[k]), k
    assert got_att["n_sup"] == plain_att["n_sup"]
    assert np.array_equal(m.predict()[0], plain_pred)                         # predictions: unweighted
    m.close()
