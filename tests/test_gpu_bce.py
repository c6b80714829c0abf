"""The sigmoid answer head on the GPU (rau_set_answer_loss, RAU_LOSS_BCE; bce_head.hip): a per-answer sigmoid with
binary cross-entropy against one-hot labels or the soft targets of an answer set, through the step path.

1. parity    losses and every gradient group against tests/bce_ref.py in fp64 (tests/test_gpu_parity.py's bar of 1e-4
             max-norm relative per tensor), SMALL / EDGE / MEDK, train and evaluate mode, labels and a set; the logits
             are bitwise those of the same step under the softmax criterion; SMALL in bf16 mode against the emulated
             reference with the bar tests/test_gpu_bf16.py derives;
2. contract  rau_criterion_backward_bce against predict.soft_bce_grad at 1e-6; unlabelled rows are +0 bits and loss 0;
             repeated calls give the same bits; extreme logits give finite results;
3. stats     rau_step_stats under the criterion: loss[:H] bitwise rau_get_losses, loss[H:] against
             predict.set_stats(loss="bce") at 1e-5, every count and rau_step_scores bitwise the softmax step's;
4. state     errors, the dropped forward, CE -> BCE -> CE against a fresh context, what survives the switch, the
             refusal of merge_w;
5. together  select_w and att_w under the criterion;
6. graph     rau_graph_step under the criterion, and no replay across a switch;
7. modules   rau_criterion_forward_bce / _backward_bce against the step, and feval(loss="bce")."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib as L
from rau_vqa_amd import predict
from tests import bce_ref, util
from tests.test_gpu_answers import MEDK, answer_set
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1
GROUPS = ("embed", "rnn", "mult")
SHAPES = {"small": (util.SMALL, 0.5), "edge": (util.EDGE, 0.5), "medk": (MEDK, 0.2)}
EXTREME = np.array([-1e4, -90, -20, 0, 20, 90, 1e4], np.float32)
COUNT_KEYS = ("loss_do_pred", "correct", "do_pred_correct", "fired", "selected")
G = 4


# ------------------------------------------------------------------------------------------ problems, references
@functools.lru_cache(maxsize=None)
def problem(name):
    """(sh, batch, params, masks, answers) of a shape, computed once and left unchanged.  The set is
    tests/test_gpu_answers.py's (row 0 a duplicate id, row 1 without entries, ids 1 and K, weights on empty entries)
    with row 0's duplicate pair summing above 1 and row 4 labelled with all weights 0."""
    dims, scale = SHAPES[name]
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, scale=scale)
    ids, w, score = answer_set(dims, G, seed=3)
    w[0, :2] = 0.75
    if ids[4, 0] == 0:
        ids[4, 0] = 2
    w[4] = 0
    return sh, batch, params, masks, (ids, w, score)


@functools.lru_cache(maxsize=None)
def reference(name, mode, target):
    sh, batch, params, masks, ans = problem(name)
    return bce_ref.step(sh, params, batch, masks if mode == "train" else None, hop_weights(sh.H),
                        answers=ans[:2] if target == "set" else None)


def hop_weights(H):
    return np.full(H, float(H), np.float32)


def make_model(name, mode="train", dtype="f32", loss=None):
    from rau_vqa_amd.model import RAU, Config
    sh, _batch, params, masks, _ans = problem(name)
    m = RAU(Config(**SHAPES[name][0], dtype=dtype))
    m.set_params(params)
    if mode == "train":
        m.training()
        m.set_masks(masks)
    else:
        m.evaluate()
    if loss is not None:
        m.set_answer_loss(loss)
    return m


def put(m, name, target="labels", **kw):
    _sh, batch, _params, _masks, ans = problem(name)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"],
                **({"answers": ans} if target == "set" else {}), **kw)


def run(m, hop_w, graph=False, stats=True, **terms):
    """zero_grads + forward + backward on the resident batch: outputs, statistics (read before the backward, as
    tests/test_gpu_answers.py does) and gradients."""
    if graph:
        m.graph_step(hop_w, zero_grads=True, **terms)
    else:
        m.zero_grads()
        m.forward()
    out = {"losses": m.losses(), "logits": m.logits(), "argmax": m.argmax(), "dopred": m.dopred()}
    if stats:
        out["stats"] = m.step_stats()
    if not graph:
        m.backward(hop_w, **terms)
    out["grads"] = m.get_grads()
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same_bits(a, b, stats=True):
    for k in ("losses", "logits", "argmax", "dopred"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for g in GROUPS:
        assert np.array_equal(bits(a["grads"][g]), bits(b["grads"][g])), g
    if stats:
        for k in ("loss",) + COUNT_KEYS:
            assert np.array_equal(bits(a["stats"][k]), bits(b["stats"][k])), k
        assert a["stats"]["did_correct"] == b["stats"]["did_correct"]


def group_errs(got, ref):
    errs = {"losses": util.rel_err(got["losses"], ref["losses"])}
    for g in GROUPS:
        errs[g] = util.rel_err(got["grads"][g], ref["g_" + g])
    return errs


def rc(m, name, *args):
    return getattr(m._lib, name)(m._h, *args)


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("target", ["labels", "set"])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", ["small", "edge", "medk"])
def test_parity_with_the_reference(name, mode, target):
    sh = problem(name)[0]
    hop_w = hop_weights(sh.H)
    m = make_model(name, mode)
    assert m.answer_loss == "ce"
    put(m, name, target)
    ce = run(m, hop_w)
    m.set_answer_loss("bce")
    assert m.answer_loss == "bce"
    got = run(m, hop_w)
    m.close()
    assert np.array_equal(bits(got["logits"]), bits(ce["logits"]))      # the forward does not depend on the loss
    assert np.array_equal(got["argmax"], ce["argmax"]) and np.array_equal(bits(got["dopred"]), bits(ce["dopred"]))
    assert not np.array_equal(got["losses"], ce["losses"])
    ref = reference(name, mode, target)
    errs = group_errs(got, ref)
    print(name, mode, target, {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"
    assert util.rel_err(got["logits"], ref["logits"]) < TOL


@pytest.mark.parametrize("target", ["labels", "set"])
def test_bf16_mode_against_the_emulated_reference(target):
    """The bar of tests/test_gpu_select.py's bf16 test, derived the same way from tests/test_gpu_bf16.py's constants:
    TOL_BASE + 2^-8 / sqrt(shortest reduction) + SAFETY x the largest shift of the nudged emulations."""
    sh, batch, params, masks, ans = problem("small")
    hop_w = hop_weights(sh.H)
    answers = ans[:2] if target == "set" else None
    m = make_model("small", dtype="bf16")
    put(m, "small", target)
    ce = run(m, hop_w)
    m.set_answer_loss("bce")
    got = run(m, hop_w)
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    assert np.array_equal(bits(got["logits"]), bits(ce["logits"]))
    with RT.bf16_emulation():
        emu = bce_ref.step(sh, params, batch, masks, hop_w, answers=answers, bf16=True)
    nudged = []
    for n in NUDGES:
        with RT.bf16_emulation(n):
            nudged.append(bce_ref.step(sh, params, batch, masks, hop_w, answers=answers, bf16=True))
    one_flip = 2.0 ** -8 / np.sqrt(min(sh.E, sh.Rq, sh.R, sh.M, sh.A, sh.S, sh.D, sh.K))
    err = lambda a, b: float(np.max(np.abs(a - b))) if np.max(np.abs(b)) < 1e-12 else util.rel_err(a, b)
    tensors = lambda r, grads: dict([("losses", r["losses"])] + [
        (nm, grads[grp][sl]) for grp in GROUPS for nm, sl in util.layer_slices(layouts[grp])])
    dev = tensors(got, got["grads"])
    t_emu = tensors(emu, {g: emu["g_" + g] for g in GROUPS})
    t_nudged = [tensors(x, {g: x["g_" + g] for g in GROUPS}) for x in nudged]
    bad, ratio = {}, 0.0
    for k in dev:
        tol = TOL_BASE + one_flip + SAFETY * max(err(x[k], t_emu[k]) for x in t_nudged)
        e = err(dev[k], t_emu[k])
        ratio = max(ratio, e / tol)
        if not e < tol:
            bad[k] = (e, tol)
    print(f"bf16 sigmoid head ({target}): largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated reference, (error, derived bar): {bad}"


# ------------------------------------------------------------------------------------------ 2. contract
class Dev:
    """Uploads through rau_dev_alloc / rau_dev_upload; downloads of ctx-owned slots."""

    def __init__(self, m):
        self.m, self.lib, self.h = m, m._lib, m._h

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        L.check(self.lib.rau_dev_alloc(self.h, a.size, C.byref(p)))
        L.check(self.lib.rau_dev_upload(self.h, p, a.ctypes.data, a.nbytes))
        return p

    def down(self, ptr, shape):
        out = np.empty(shape, np.float32)
        L.check(self.lib.rau_dev_download(self.h, out.ctypes.data, C.c_void_p(ptr), out.nbytes))
        return out

    def criterion(self, h, lg_d, labels_d, Gn, ids_d, w_d, scale=1.0):
        """(loss, d_logits [B, K]) of the two module-level calls"""
        c = self.m.cfg
        loss, q = C.c_float(), C.c_void_p()
        L.check(self.lib.rau_criterion_forward_bce(self.h, h, lg_d, labels_d, Gn, ids_d, w_d, C.byref(loss)))
        L.check(self.lib.rau_criterion_backward_bce(self.h, h, lg_d, labels_d, Gn, ids_d, w_d, scale, C.byref(q)))
        return np.float32(loss.value), self.down(q.value, (self.m.batch_size, c.K))


@pytest.mark.parametrize("name", ["small", "medk"])
def test_module_calls_are_the_numpy_statement(name):
    sh, batch, _params, _masks, (ids, w, _score) = problem(name)
    B, K = sh.B, sh.K
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((B, K)) * 3).astype(np.float32)
    x[0, :EXTREME.size] = EXTREME              # row 0 carries the duplicate pair: a target of 1 among the extremes
    x[1, -EXTREME.size:] = EXTREME             # the row without entries
    x[2, :EXTREME.size] = EXTREME[::-1]
    ids = ids.copy()
    ids[0, :2] = 1                             # ... on the logit -1e4
    ids[2, 0] = EXTREME.size                   # id 7: the logit -1e4 of row 2
    m = make_model(name, "eval")
    d = Dev(m)
    lg_d, ids_d, w_d, y_d = d.up(x), d.up(ids), d.up(w), d.up(batch["labels"])
    for kind in ("ce", "bce"):                 # the calls do not read the context's switch
        m.set_answer_loss(kind)
        loss, dl = d.criterion(0, lg_d, None, G, ids_d, w_d)
        assert np.isfinite(loss) and np.isfinite(dl).all()
        _rows, want_loss = predict.soft_bce(x, ids, w)
        want = predict.soft_bce_grad(x, ids, w)
        errs = {"grad": util.rel_err(dl, want), "loss": abs(float(loss) - float(want_loss)) / float(want_loss)}
        print(name, kind, errs)
        assert errs["grad"] <= 1e-6, errs
        # the loss: the same terms to a few ulp of expf / log1pf, summed in the same order
        assert errs["loss"] <= 1e-6, errs
        assert not bits(dl[1]).any()                                   # the row without entries: +0 bits
        assert (dl[4] > 0).all()                                       # all weights 0: every answer pushed down
        assert predict.bce_target(ids, w, K)[0, 0] == 1                # the duplicate pair, clamped
        assert dl[0, 0] == -(np.float32(1) / np.float32(B))            # (sigmoid(-1e4) - 1) / B = -1 / B exactly
        loss2, dl2 = d.criterion(0, lg_d, None, G, ids_d, w_d)         # repeated calls: the same bits
        assert loss2 == loss and np.array_equal(bits(dl2), bits(dl))
        _l, dl3 = d.criterion(0, lg_d, None, G, ids_d, w_d, scale=2.0)
        assert np.array_equal(dl3, dl * np.float32(2))
        # labels: the one-entry sets of weight 1
        loss_y, dl_y = d.criterion(sh.H - 1, lg_d, y_d, 0, None, None)
        yi, yw = batch["labels"][:, None], np.ones((B, 1), np.float32)
        assert util.rel_err(dl_y, predict.soft_bce_grad(x, yi, yw)) <= 1e-6
        assert abs(float(loss_y) - float(predict.soft_bce(x, yi, yw)[1])) <= 1e-6 * float(loss_y)
        assert np.isfinite(dl_y).all()
    # no row has an entry: loss exactly 0, every gradient +0
    none_d = d.up(np.zeros((B, G), np.int32))
    loss0, dl0 = d.criterion(0, lg_d, None, G, none_d, w_d)
    assert loss0 == 0 and not np.signbit(loss0) and not bits(dl0).any()
    assert rc(m, "rau_criterion_forward_bce", 0, lg_d, None, G, None, None, None) == INVALID
    assert rc(m, "rau_criterion_forward_bce", 0, lg_d, None, 17, ids_d, w_d, None) == INVALID
    assert rc(m, "rau_criterion_forward_bce", sh.H, lg_d, y_d, 0, None, None, None) == INVALID
    m.close()


# ------------------------------------------------------------------------------------------ 3. stats
@pytest.mark.parametrize("name,mode", [("small", "train"), ("medk", "eval")])
@pytest.mark.parametrize("target", ["labels", "set"])
def test_step_stats_under_the_sigmoid_criterion(name, mode, target):
    sh, batch, _params, _masks, (ids, w, score) = problem(name)
    H = sh.H
    m = make_model(name, mode)
    put(m, name, target)
    m.forward()
    ce = m.step_stats()
    ce_scores = m.step_scores() if target == "set" else None
    m.set_answer_loss("bce")
    m.forward()
    st = m.step_stats()
    assert np.array_equal(bits(st["loss"][:H]), bits(m.losses()))
    for k in COUNT_KEYS:
        assert np.array_equal(bits(st[k]), bits(ce[k])), k
    assert st["did_correct"] == ce["did_correct"]
    if target == "set":
        sc = m.step_scores()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(sc, ce_scores))
        want = predict.set_stats(m.logits(), m.dopred(), ids, w, score, loss="bce")
    else:
        y = batch["labels"][:, None]
        want = predict.set_stats(m.logits(), m.dopred(), y, np.ones(y.shape, np.float32), loss="bce")
    m.close()
    err = np.abs(st["loss"].astype(np.float64) - want["loss"]) / np.abs(want["loss"])
    print(name, mode, target, err)
    assert (err[H:] <= 1e-5).all() and (err[:H] <= 1e-5).all(), err
    assert not np.array_equal(st["loss"][H:], ce["loss"][H:])


# ------------------------------------------------------------------------------------------ 4. state
def test_errors_and_the_dropped_forward():
    sh = problem("small")[0]
    hop_w = hop_weights(sh.H)
    m = make_model("small")
    put(m, "small", "set")
    assert rc(m, "rau_set_answer_loss", 2) == INVALID and rc(m, "rau_set_answer_loss", -1) == INVALID
    assert m.answer_loss == "ce"
    with pytest.raises(ValueError):
        m.set_answer_loss("hinge")
    m.zero_grads()
    m.forward()
    m.set_answer_loss("ce")                     # not a change: the forward stays
    m.step_stats()
    m.set_answer_loss("bce")
    buf = np.zeros(4 * sh.H + 3, np.float32)
    p = buf.ctypes.data
    assert rc(m, "rau_backward", hop_w.ctypes.data) == STATE
    assert rc(m, "rau_backward_select", hop_w.ctypes.data, hop_w.ctypes.data) == STATE
    assert rc(m, "rau_step_stats", p, None, None) == STATE
    assert rc(m, "rau_step_scores", None, p) == STATE
    assert all(not g.any() for g in m.get_grads().values())            # nothing launched
    m.forward()
    m.step_stats()
    m.backward(hop_w)
    m.close()


def test_ce_bce_ce_gives_the_bits_of_a_context_never_switched():
    sh = problem("small")[0]
    hop_w = hop_weights(sh.H)
    fresh = make_model("small")
    put(fresh, "small", "set")
    want = run(fresh, hop_w)
    fresh.close()
    fresh = make_model("small", loss="bce")
    put(fresh, "small", "set")
    want_bce = run(fresh, hop_w)
    fresh.close()
    m = make_model("small")
    put(m, "small", "set")
    same_bits(run(m, hop_w), want)
    m.set_answer_loss("bce")
    same_bits(run(m, hop_w), want_bce)
    m.set_answer_loss("ce")
    same_bits(run(m, hop_w), want)
    m.close()


def test_set_counts_and_bank_survive_the_switch():
    sh, batch, _params, _masks, ans = problem("small")
    hop_w = hop_weights(sh.H)
    counts = np.array([12, 7, 3, 1, 5, 12, 2, 9], np.int32)
    rows = np.arange(sh.B, dtype=np.int32)[::-1].copy()
    results = []
    for switch in (False, True):
        m = make_model("small", loss=None if switch else "bce")
        m.bank_create(sh.B + 2)
        m.bank_put(1, batch["feats"])
        m.set_batch(None, batch["tokens"], batch["lens"], batch["labels"], bank_rows=rows + 1, answers=ans,
                    regions=counts)
        if switch:
            m.forward()
            m.set_answer_loss("bce")
            assert m.batch_answers == G and m.batch_regions
            assert m.bank_info() == {"capacity": sh.B + 2, "feat_type": "f32", "rows_filled": sh.B}
            assert np.array_equal(m.bank_get(1, sh.B), batch["feats"].reshape(sh.B, sh.D, sh.S))
        results.append(run(m, hop_w))           # no new upload: the batch, its set and its counts are still there
        m.close()
    same_bits(*results)


def test_merged_training_is_refused_under_the_sigmoid_criterion():
    sh = problem("small")[0]
    hop_w = hop_weights(sh.H)
    mw, zeros = np.array([0.7, 1.3], np.float32), np.zeros(2, np.float32)
    m = make_model("small", loss="bce")
    put(m, "small", "set")
    m.zero_grads()
    m.forward()
    args = (hop_w.ctypes.data, None, None)
    assert rc(m, "rau_backward_merged", *args, mw.ctypes.data) == INVALID
    assert b"RAU_LOSS_BCE" in m._lib.rau_last_error()
    assert rc(m, "rau_graph_step_merged", *args, mw.ctypes.data, 1) == INVALID
    assert all(not g.any() for g in m.get_grads().values())            # gradients untouched
    L.check(rc(m, "rau_backward_merged", *args, zeros.ctypes.data))    # the forward is still there
    g_zero = m.get_grads()
    m.zero_grads()
    m.forward()
    L.check(rc(m, "rau_backward_merged", *args, None))
    g_null = m.get_grads()
    m.zero_grads()
    m.forward()
    m.backward(hop_w)
    g_plain = m.get_grads()
    for g in GROUPS:
        assert np.array_equal(bits(g_zero[g]), bits(g_null[g])) and np.array_equal(bits(g_null[g]), bits(g_plain[g]))
    m.set_answer_loss("ce")                      # and under the softmax criterion the term is there as before
    m.zero_grads()
    m.forward()
    L.check(rc(m, "rau_backward_merged", *args, mw.ctypes.data))
    m.close()


# ------------------------------------------------------------------------------------------ 5. together
@pytest.mark.parametrize("target", ["labels", "set"])
def test_select_head_under_the_sigmoid_criterion(target):
    from tests.test_gpu_select import check_argmax, grad_errs, small_answer_set, targets
    from tests.test_gpu_select import make_model as select_model
    from tests.test_gpu_select import problem as select_problem
    sh, batch, params, masks = select_problem("SMALL")      # labels that the hop-0 answer hits on the even rows
    ans = small_answer_set(batch, sh) if target == "set" else None
    hop_w, select_w = [3, 3, 3], [0.7, 0.4, 1.3]
    m = select_model(sh, params, masks)
    m.set_answer_loss("bce")
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"],
                **({} if ans is None else {"answers": ans}))
    m.zero_grads()
    m.forward()
    fwd = bce_ref.step(sh, params, batch, masks, hop_w, backward=False)
    t_gt = targets(check_argmax(m, fwd), batch, ans)
    assert t_gt.any() and not t_gt.all()
    m.backward(hop_w, select_w=select_w)
    got = m.get_grads()
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    ref = bce_ref.step(sh, params, batch, masks, hop_w, select_w, t_gt, None if ans is None else ans[:2])
    errs = grad_errs(got, ref, layouts)
    print(target, {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"


def test_attention_supervision_adds_what_it_adds_under_the_softmax_criterion():
    """The attention term does not read the answer criterion and the forward is the same, so
    grads(BCE, att_w) = grads(BCE) + (grads(CE, att_w) - grads(CE)) up to rounding: within TOL of the largest of
    the four per group."""
    from tests.test_gpu_att_targets import att_weights, reference as att_reference
    sh, batch, params, masks, t, _n, _ref = att_reference("small")
    from rau_vqa_amd.model import RAU, Config
    hop_w, att_w = hop_weights(sh.H), att_weights(sh.H)
    m = RAU(Config(**util.SMALL))
    m.set_params(params)
    m.training()
    m.set_masks(masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], att_targets=t)
    res = {}
    for kind in ("ce", "bce"):
        m.set_answer_loss(kind)
        res[kind, False] = run(m, hop_w, stats=False)["grads"]
        res[kind, True] = run(m, hop_w, stats=False, att_w=att_w)["grads"]
    m.close()
    for g in GROUPS:
        f64 = lambda a: a.astype(np.float64)
        want = f64(res["bce", False][g]) + (f64(res["ce", True][g]) - f64(res["ce", False][g]))
        den = max(np.max(np.abs(res[k][g])) for k in res)
        e = np.max(np.abs(res["bce", True][g] - want)) / den
        print(g, f"{e:.1e}")
        assert e < TOL, g
    assert not np.array_equal(res["bce", True]["mult"], res["bce", False]["mult"])


# ------------------------------------------------------------------------------------------ 6. graph
def test_graph_step_is_the_eager_step_and_never_replays_the_other_kind():
    sh = problem("small")[0]
    hop_w = hop_weights(sh.H)
    m = make_model("small")
    put(m, "small", "set")
    eager_ce = run(m, hop_w)
    m.set_answer_loss("bce")
    eager_bce = run(m, hop_w)
    assert not np.array_equal(eager_bce["grads"]["mult"], eager_ce["grads"]["mult"])
    m.set_answer_loss("ce")
    same_bits(run(m, hop_w, graph=True), eager_ce)          # captured under the softmax criterion
    m.set_answer_loss("bce")
    same_bits(run(m, hop_w, graph=True), eager_bce)         # the sigmoid results, not a replay
    same_bits(run(m, hop_w, graph=True), eager_bce)         # ... and their replay
    m.set_answer_loss("ce")
    same_bits(run(m, hop_w, graph=True), eager_ce)          # back: the captured softmax step's bits
    m.close()


# ------------------------------------------------------------------------------------------ 7. module level
@pytest.mark.parametrize("target", ["labels", "set"])
def test_module_calls_equal_the_step(target):
    from rau_vqa_amd import modules
    sh, batch, _params, _masks, (ids, w, _score) = problem("small")
    H, B, K = sh.H, sh.B, sh.K
    hop_w = hop_weights(H)
    m = make_model("small", loss="bce")
    put(m, "small", target)
    step = run(m, hop_w, stats=False)
    d = Dev(m)
    ids_d, w_d, y_d = d.up(ids), d.up(w), d.up(batch["labels"])
    tgt = (None, G, ids_d, w_d) if target == "set" else (y_d, 0, None, None)
    for kind in ("bce", "ce"):                  # whichever kind the context is switched to
        m.set_answer_loss(kind)
        for h in range(H):
            lg_d = d.up(step["logits"][h])
            loss, dl = d.criterion(h, lg_d, *tgt)
            assert loss == step["losses"][h], (kind, h)
            yi, yw = (ids, w) if target == "set" else (batch["labels"][:, None], np.ones((B, 1), np.float32))
            assert util.rel_err(dl, predict.soft_bce_grad(step["logits"][h], yi, yw)) <= 1e-6
    # feval over the module-level calls: the step's gradients at tests/test_gpu_modules.py's bar for the two paths
    cuda = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a)).cuda().to(dt or torch.float32)
    m.zero_grads()
    y = cuda(batch["labels"], torch.int32) if target == "labels" else None
    answers = (cuda(ids, torch.int32), cuda(w)) if target == "set" else None
    losses, _answers = modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32),
                                     cuda(batch["lens"], torch.int32), y, hop_w, loss="bce", answers=answers)
    m.sync()
    g_mod = m.get_grads()
    m.close()
    assert util.rel_err(losses.numpy(), step["losses"]) < 1e-5
    for g in GROUPS:
        assert util.rel_err(g_mod[g], step["grads"][g]) < 1e-5, g
