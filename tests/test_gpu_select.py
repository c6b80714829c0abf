"""The step-selection head's gradient in the step-level backward (rau_backward_select,
rau_graph_step_select, select_bwd.hip): the multiplier of the reference's d_do_pred:mul(0) (SS:566) as a
per-hop argument.

The oracle: oracle/ref_torch.py's _step restated below (its forty lines, on ref_torch's own multimodal,
deep_lstm, _drop, _split and specs) with  sum_h select_w[h] * BCE_eps(do_pred_h, t_h)  added to the loss, in
fp64 with explicit masks.  t_h = do_pred_gt comes from the DEVICE's argmax of that forward, after the test
has asserted that this argmax equals the oracle's on every row and hop (the seeds' top-2 margins are at least
1e-4 relative in fp64, ten times util.argmax_margin_ok's bar: checked on the CPU before they were committed).
Bar: TOL = 1e-4, util.rel_err per layer slice, as tests/test_gpu_parity.py.

bf16 mode: the bar is the one tests/test_gpu_bf16.py derives against the emulated oracle.  Its derivation
lives inside that module's run(), which runs its own (select-free) step, so it cannot be called; its
constants TOL_BASE, NUDGES and SAFETY are imported (the import has no side effects) and the derivation --
TOL_BASE + 2^-8 / sqrt(shortest reduction) + SAFETY x the largest shift of the nudged emulations -- is
restated here around the restated loop.
"""
import numpy as np
import pytest
import torch

from oracle import ref_torch as RT
from oracle.ref_torch import _drop, _split, deep_lstm, mult_specs, multimodal, rnn_specs
from tests import util
from tests.test_gpu_bf16 import NUDGES, SAFETY, TOL_BASE

pytestmark = pytest.mark.gpu

TOL = 1e-4
STATE, INVALID = -3, -1
SCALE = {"SMALL": 0.5, "EDGE": 0.5, "MEDIUM": 0.2}
GROUPS = ("embed", "rnn", "mult")


# ------------------------------------------------------------------------------------------ the oracle
def oracle_step(sh, params, batch, masks, hop_w, select_w, t_gt, answers=None, bf16=False):
    """ref_torch._step with the select term.  t_gt [H, B] 0/1 (None: forward only); answers = (ids, w): the
    CE is predict.soft_ce's, sum_g w (lse - logit[y_g]) over the non-empty entries, mean over the batch."""
    dtype = torch.float64
    t = lambda a: torch.as_tensor(a).to(dtype)
    flat = {k: t(params[k]).clone().requires_grad_(True) for k in GROUPS}
    Emb = flat["embed"].view(sh.V, sh.E)
    Pr = _split(flat["rnn"], rnn_specs(sh))
    Pm = _split(flat["mult"], mult_specs(sh))
    feats4d = t(batch["feats"]).reshape(sh.B, sh.D, sh.S, 1)
    tokens = torch.as_tensor(batch["tokens"]).long()
    lens = torch.as_tensor(batch["lens"]).long()
    mk = lambda k: None if masks is None else torch.as_tensor(masks[k])
    m_we, m_rnn, m_q, m_x, m_mf = mk("we"), mk("rnn"), mk("q"), mk("x"), mk("mf")
    B, Q = sh.B, 4 * sh.Rq
    state = torch.zeros(B, Q, dtype=dtype)
    q = torch.zeros(B, Q, dtype=dtype)
    for tt in range(1, int(lens.max()) + 1):
        we = torch.tanh(_drop(Emb[tokens[tt - 1] - 1], None if m_we is None else m_we[tt - 1], sh.p_we))
        state = deep_lstm(sh, Pr, we, state, None if m_rnn is None else m_rnn[tt - 1])
        q = torch.where((lens == tt).unsqueeze(1), state, q)
    c = torch.zeros(B, sh.R, dtype=dtype)
    h = torch.zeros(B, sh.R, dtype=dtype)
    y = torch.as_tensor(batch["labels"]).long() - 1
    if answers is not None:
        ids = torch.as_tensor(answers[0]).long()
        aw = torch.where(ids > 0, t(answers[1]), torch.zeros((), dtype=dtype))
    logits, dopred, total = [], [], 0.0
    eps = 1e-12
    for hop in range(sh.H):
        score, dp, _a, c, h = multimodal(
            sh, Pm, q, feats4d, c, h,
            None if m_q is None else m_q[hop],
            None if m_x is None else m_x[hop].reshape(sh.B, sh.D, sh.S, 1),
            None if m_mf is None else m_mf[hop], bf16=bf16)
        logits.append(score.detach().numpy())
        dopred.append(dp.detach().numpy())
        if t_gt is None:
            continue
        if answers is None:
            loss = torch.nn.functional.cross_entropy(score, y)
        else:
            lse = torch.logsumexp(score, dim=1, keepdim=True)
            loss = (aw * (lse - torch.gather(score, 1, (ids - 1).clamp(min=0)))).sum() / B
        tg = t(t_gt[hop])
        bce = -(tg * torch.log(dp + eps) + (1 - tg) * torch.log(1 - dp + eps)).mean()
        total = total + float(hop_w[hop]) * loss + float(select_w[hop]) * bce
    res = {"logits": np.stack(logits), "dopred": np.stack(dopred)}
    res["argmax"] = np.argmax(res["logits"], axis=-1) + 1
    if t_gt is not None:
        total.backward()
        for k in GROUPS:
            res["g_" + k] = flat[k].grad.numpy()
    return res


def targets(argmax, batch, answers=None):
    """do_pred_gt [H, B] of rau_step_stats: argmax == label, or (set) the answer carries a positive score."""
    if answers is None:
        return (argmax == batch["labels"][None, :]).astype(np.float32)
    ids, _w, score = answers
    hit = (ids[None, :, :] == argmax[:, :, None]) & (ids[None, :, :] > 0)
    return ((hit * score[None, :, :]).sum(-1) > 0).astype(np.float32)


# ------------------------------------------------------------------------------------------ the device
def make_model(sh, params, masks=None, dtype="f32"):
    from rau_vqa_amd.model import RAU, Config
    cfg = Config(**{k: getattr(sh, k) for k in
                    ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H",
                     "p_we", "p_rnn", "p_q", "p_x", "p_mf")}, dtype=dtype)
    m = RAU(cfg)
    m.set_params(params)
    m.training()
    if masks is not None:
        m.set_masks(masks)
    return m


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def step(m, hop_w, select_w, how="eager"):
    """zero_grads + forward + backward through the named entry point; returns the three gradient vectors.
    select_w None is passed as NULL to the *_select entry points (how = 'select' | 'graph_select')."""
    hw = f32(hop_w)
    sw = None if select_w is None else f32(select_w)
    sp = None if sw is None else sw.ctypes.data
    lib, h = m._lib, m._h
    from rau_vqa_amd._lib import check
    if how in ("graph", "graph_select"):
        if how == "graph":
            check(lib.rau_graph_step(h, hw.ctypes.data, 1))
        else:
            check(lib.rau_graph_step_select(h, hw.ctypes.data, sp, 1))
    else:
        m.zero_grads()
        m.forward()
        if how == "plain":
            check(lib.rau_backward(h, hw.ctypes.data))
        else:
            check(lib.rau_backward_select(h, hw.ctypes.data, sp))
    return m.get_grads()


def grad_errs(got, ref, layouts):
    errs = {}
    for grp in layouts:
        for name, sl in util.layer_slices(layouts[grp]):
            r = ref["g_" + grp][sl]
            if np.max(np.abs(r)) < 1e-12:
                errs[name] = float(np.max(np.abs(got[grp][sl] - r)))
            else:
                errs[name] = util.rel_err(got[grp][sl], r)
    return errs


def same_bits(a, b):
    for k in GROUPS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def check_argmax(m, ref_fwd, margin=1e-5):
    """The device's argmax, asserted equal to the oracle's on EVERY row and hop."""
    am = m.argmax()
    ok, decided, total = util.argmax_margin_ok(ref_fwd["logits"], am, ref_fwd["argmax"], margin=margin)
    assert decided == total, f"{total - decided} rows within the margin: choose another seed"
    assert ok and np.array_equal(am, ref_fwd["argmax"])
    return am


_PROBLEMS = {}


def problem(dims_name):
    """util.make_problem at the shape's committed scale, computed once and shared, with the labels of the even
    rows set to the fp64 oracle's hop-0 answer under the explicit masks: the forward does not read the labels,
    and a target that is 0 on every row would leave half of the BCE gradient untested."""
    if dims_name not in _PROBLEMS:
        sh = util.shapes(getattr(util, dims_name))
        batch, params, masks = util.make_problem(sh, scale=SCALE[dims_name])
        fwd = oracle_step(sh, params, batch, masks, None, None, None)
        batch["labels"] = batch["labels"].copy()
        batch["labels"][::2] = fwd["argmax"][0, ::2]
        _PROBLEMS[dims_name] = (sh, batch, params, masks)
    sh, batch, params, masks = _PROBLEMS[dims_name]
    return sh, dict(batch), params, masks


def parity(dims_name, hop_w, select_w, lens=None, answers=None, philox=False, how="select"):
    """Device step against the oracle at TOL; returns (errs, layouts, device grads, oracle result, targets)."""
    sh, batch, params, masks = problem(dims_name)
    if lens is not None:
        batch["lens"] = lens
    m = make_model(sh, params, None if philox else masks)
    put = lambda: m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"],
                              **({} if answers is None else {"answers": answers}))
    if philox:   # the device draws the masks; the oracle is fed what rau_get_mask reads back
        m.set_dropout_seed(11, 5)
        put()
        m.forward()   # (hits for the even rows under THESE masks, as problem() arranges under the explicit ones)
        batch["labels"] = batch["labels"].copy()
        batch["labels"][::2] = m.argmax()[0, ::2]
        m.set_dropout_seed(11, 5)
    put()
    got = step(m, hop_w, select_w, how)
    if philox:
        masks = {k: m.get_mask(k) for k in ("we", "rnn", "q", "x", "mf")}
    am = check_argmax(m, oracle_step(sh, params, batch, masks, hop_w, select_w, None))
    t_gt = targets(am, batch, answers)
    ref = oracle_step(sh, params, batch, masks, hop_w, select_w, t_gt,
                      None if answers is None else answers[:2])
    layouts = {k: m.layout(k) for k in GROUPS}
    m.close()
    errs = grad_errs(got, ref, layouts)
    print({k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"
    return errs, layouts, got, ref, t_gt


def head_slices(layouts):
    """The head's two tensors in the mult group's layout: classifier.out_do_pred.{weight,bias}."""
    return {n.split(".", 1)[1]: sl for n, sl in util.layer_slices(layouts["mult"]) if ".out_do_pred." in n}


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("dims_name,hop_w,select_w", [
    ("SMALL", [3, 3, 3], [0.7, 0, 1.3]),
    ("EDGE", [1], [0.9]),
])
def test_label_batch_against_the_oracle(dims_name, hop_w, select_w):
    _errs, layouts, got, ref, t_gt = parity(dims_name, hop_w, select_w)
    hs = head_slices(layouts)
    assert sorted(hs) == ["out_do_pred.bias", "out_do_pred.weight"]
    for n, sl in hs.items():   # the head's own gradient is there (and was inside the bar above)
        assert np.max(np.abs(ref["g_mult"][sl])) > 1e-6 and np.any(got["mult"][sl] != 0), n
    assert 0 < t_gt.sum() < t_gt.size   # both target values occur


# ------------------------------------------------------------------------------------------ 2. select only
@pytest.mark.parametrize("hop_w,select_w", [
    ([0, 0, 0], [1, 1, 1]),
    ([3, 0, 0], [0, 0, 1]),     # the active range is set by select_w
    ([3, 3, 0], [1, 0, 0]),     # the trailing hop is skipped
])
def test_select_only_and_the_active_range(hop_w, select_w):
    parity("SMALL", hop_w, select_w)


# ------------------------------------------------------------------------------------------ 3. unchanged path
def test_null_and_zero_select_weights_are_rau_backward_bit_for_bit():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    hop_w = [3, 3, 3]
    base = step(m, hop_w, None, "plain")
    same_bits(step(m, hop_w, None, "select"), base)
    same_bits(step(m, hop_w, [0, 0, 0], "select"), base)
    same_bits(step(m, hop_w, None, "graph_select"), base)
    same_bits(step(m, hop_w, [0, 0, 0], "graph_select"), base)
    assert any(not np.array_equal(step(m, hop_w, [0, 1, 0], "select")[k], base[k]) for k in GROUPS)
    m.close()


# ------------------------------------------------------------------------------------------ 4. answer sets
def small_answer_set(batch, sh):
    """G = 3: the label first (so hits occur), two more ids; row 1 has no entry, row 2's label entry has
    score 0 (a hit that does not count), row 3 repeats its label (duplicates add up)."""
    rng = np.random.RandomState(5)
    ids = rng.randint(1, sh.K + 1, size=(sh.B, 3)).astype(np.int32)
    ids[:, 0] = batch["labels"]
    w = rng.uniform(0.1, 1.0, size=(sh.B, 3)).astype(np.float32)
    score = np.minimum(rng.randint(1, 5, size=(sh.B, 3)) / np.float32(3), 1).astype(np.float32)
    ids[1, :] = 0
    score[2, 0] = 0
    score[2, ids[2] == ids[2, 0]] = 0
    ids[3, 2] = ids[3, 0]
    ids[4, 1] = 0
    return ids, w, score


def test_answer_set_targets_and_gradients():
    sh, batch, params, masks = problem("SMALL")
    ans = small_answer_set(batch, sh)
    _errs, _lay, _got, _ref, t_gt = parity("SMALL", [3, 3, 3], [0.7, 0.4, 1.3], answers=ans)
    assert not t_gt[:, 1].any()      # a row without entries is never "correct"
    assert not t_gt[:, 2].any()      # nor one whose only possible hit has score 0
    # and the set rule is what rau_step_stats counts (correct[h] = sum of the targets)
    m = make_model(sh, params, masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"], answers=ans)
    m.forward()
    assert np.array_equal(m.step_stats()["correct"][:sh.H], t_gt.sum(1).astype(np.int64))
    m.close()


# ------------------------------------------------------------------------------------------ 5. MEDIUM
def test_medium_ragged_with_device_masks():
    sh = util.shapes(util.MEDIUM)
    lens = np.random.RandomState(2).randint(1, sh.T + 1, size=sh.B).astype(np.int32)
    lens[7] = 0
    lens[-1] = sh.T
    parity("MEDIUM", [2, 2], [0.8, 1.1], lens=lens, philox=True)


# ------------------------------------------------------------------------------------------ 6. graph
def test_graph_step_select_replays_with_new_weights():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    hop_w = [3, 3, 3]
    for sw in ([0.7, 0, 1.3], [0.2, 0.5, 2.0]):     # capture, then a replay at other non-zero values
        same_bits(step(m, hop_w, sw, "graph_select"), step(m, hop_w, sw, "select"))
    same_bits(step(m, hop_w, [0, 0, 0], "graph_select"), step(m, hop_w, None, "plain"))
    same_bits(step(m, hop_w, [0.7, 0, 1.3], "graph_select"), step(m, hop_w, [0.7, 0, 1.3], "select"))
    m.close()


# ------------------------------------------------------------------------------------------ 7. module path
def test_module_level_feval_trains_the_same_head():
    from rau_vqa_amd import modules
    sh, batch, params, masks = problem("SMALL")
    hop_w, select_w = [3, 3, 3], [0.7, 0, 1.3]
    m = make_model(sh, params, masks)
    layouts = {k: m.layout(k) for k in GROUPS}
    cuda = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a)).cuda().to(dt or torch.float32)
    m.zero_grads()
    _losses, answers = modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32),
                                     cuda(batch["lens"], torch.int32), cuda(batch["labels"], torch.int32),
                                     f32(hop_w), select_w=f32(select_w))
    m.sync()
    g_mod = m.get_grads()
    am = answers.cpu().numpy()
    fwd = oracle_step(sh, params, batch, masks, hop_w, select_w, None)
    assert np.array_equal(am, fwd["argmax"])
    ref = oracle_step(sh, params, batch, masks, hop_w, select_w, targets(am, batch))
    bad = {k: v for k, v in grad_errs(g_mod, ref, layouts).items() if not v < TOL}
    assert not bad, f"module-level feval above {TOL}: {bad}"
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    g_step = step(m, hop_w, select_w, "select")
    bad = {k: v for k, v in grad_errs(g_step, ref, layouts).items() if not v < TOL}
    assert not bad, f"step-level above {TOL}: {bad}"
    for grp in GROUPS:   # hence the two device paths agree within 2 TOL
        for n, sl in util.layer_slices(layouts[grp]):
            den = np.max(np.abs(ref["g_" + grp][sl]))
            assert np.max(np.abs(g_mod[grp][sl] - g_step[grp][sl])) < 2 * TOL * (den if den >= 1e-12 else 1.0), n
    m.close()


# ------------------------------------------------------------------------------------------ 8. bf16 mode
def test_bf16_mode_against_the_emulated_oracle():
    sh, batch, params, masks = problem("SMALL")
    hop_w, select_w = [3, 3, 3], [0.7, 0, 1.3]
    m = make_model(sh, params, masks, dtype="bf16")
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    got = step(m, hop_w, select_w, "select")
    layouts = {k: m.layout(k) for k in GROUPS}
    with RT.bf16_emulation():
        fwd = oracle_step(sh, params, batch, masks, hop_w, select_w, None, bf16=True)
    am = check_argmax(m, fwd, margin=5e-3)
    m.close()
    t_gt = targets(am, batch)
    with RT.bf16_emulation():
        emu = oracle_step(sh, params, batch, masks, hop_w, select_w, t_gt, bf16=True)
    nudged = []
    for n in NUDGES:
        with RT.bf16_emulation(n):
            nudged.append(oracle_step(sh, params, batch, masks, hop_w, select_w, t_gt, bf16=True))
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
    print(f"bf16 select: largest error / derived bar {ratio:.2f}")
    assert not bad, f"vs emulated oracle, (error, derived bar): {bad}"
    hs = head_slices(layouts)
    assert all(np.any(got["mult"][sl] != 0) for sl in hs.values())


# ------------------------------------------------------------------------------------------ 9. determinism, errors
def test_determinism_and_refusals():
    sh, batch, params, masks = problem("SMALL")
    m = make_model(sh, params, masks)
    lib, h = m._lib, m._h
    args = (batch["feats"], batch["tokens"], batch["lens"])
    m.set_batch(*args, batch["labels"])
    hop_w, sw = f32([3, 3, 3]), f32([0.7, 0, 1.3])
    first = step(m, hop_w, sw, "select")
    same_bits(step(m, hop_w, sw, "select"), first)
    base = step(m, hop_w, None, "plain")

    def plain_still_works():
        m.set_batch(*args, batch["labels"])
        same_bits(step(m, hop_w, None, "plain"), base)

    # a batch without labels
    m.set_batch(*args, None)
    m.forward()
    assert lib.rau_backward_select(h, hop_w.ctypes.data, sw.ctypes.data) == STATE
    assert lib.rau_graph_step_select(h, hop_w.ctypes.data, sw.ctypes.data, 1) == STATE
    plain_still_works()
    # the slot that forward read has been uploaded into since
    m.set_batch(*args, batch["labels"])
    m.forward()
    m.set_batch(*args, batch["labels"])
    assert lib.rau_backward_select(h, hop_w.ctypes.data, sw.ctypes.data) == STATE
    plain_still_works()
    # non-finite weights
    m.set_batch(*args, batch["labels"])
    m.forward()
    for bad_w in (f32([0.7, np.nan, 1.3]), f32([np.inf, 0, 0])):
        assert lib.rau_backward_select(h, hop_w.ctypes.data, bad_w.ctypes.data) == INVALID
        assert lib.rau_graph_step_select(h, hop_w.ctypes.data, bad_w.ctypes.data, 1) == INVALID
    assert lib.rau_backward_select(h, bad_w.ctypes.data, sw.ctypes.data) == INVALID
    plain_still_works()
    # one backward per forward holds for the new entry point too
    m.zero_grads()
    m.forward()
    assert lib.rau_backward_select(h, hop_w.ctypes.data, sw.ctypes.data) == 0
    assert lib.rau_backward_select(h, hop_w.ctypes.data, sw.ctypes.data) == STATE
    same_bits(m.get_grads(), first)
    m.close()
