"""Answer sets on the GPU (rau_set_answers, ce_set.hip, hop_merge.hip): the criterion head, the statistics and
the metric scores against multi-answer ground truth.

1. identity   one entry of weight 1 per row gives the label path's bits;
2. parity     loss and every gradient are linear in the one-hot target and the forward does not depend on it, so
              the float64 expectation is (1/B) sum_b sum_g w[b,g] (.) over one-sample runs of the unchanged
              oracle; bar: tests/test_gpu_parity.py's 1e-4 max-norm relative per tensor;
3. stats      rau_step_stats / rau_step_scores / rau_predict_scores against predict.py's numpy statement;
4. state      lifetime of a set, errors, the asynchronous path, image-table and bank batches;
5. graph      rau_graph_step with a set;
6. modules    rau_criterion_forward_set / _backward_set against the step."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from rau_vqa_amd import _lib as L
from rau_vqa_amd import predict
from tests import util

pytestmark = pytest.mark.gpu

TOL = 1e-4
STATE, INVALID = -3, -1
STAT_KEYS = ("loss", "loss_do_pred", "correct", "do_pred_correct", "fired", "selected")
# MEDIUM's head widths at 8 samples and K = 1000 (not a multiple of the 256-thread workgroup).  It is also the
# shape at which the classifier GEMM hands MORE THAN ONE K-split partial to the head kernel: out_score is
# [H*B, K] = mf [H*B, M] Wc^T with inner dimension M = 136; gemm_lin's deferred path takes
# min(target / tiles, nk / 2) splits with nk = ceil(136 / 32) = 5 or ceil(136 / 16) = 9 stages of the skinny
# tiles and 16 column tiles, i.e. 2 or 3 partials (SMALL's M = 40 and EDGE's M = 4 give nk / 2 <= 1: one partial).
MEDK = dict(B=8, T=9, V=300, E=200, Rq=64, D=72, S=196, M=136, A=132, R=68, K=1000, H=2)
STATS = dict(B=37, T=6, V=50, E=8, Rq=16, D=24, S=49, M=40, A=20, R=16, K=12, H=3)


def make(dims, dtype="f32", seed=123, scale=0.5):
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, seed=seed, scale=scale)
    m = RAU(Config(**dims, dtype=dtype))
    m.set_params(params)
    return m, sh, batch, params, masks


def answer_set(dims, G, seed=0, counts=True):
    """ids [B, G] with: row 0 a duplicate id, row 1 without entries, ids 1 and K present, empty entries that
    carry a weight; per-sample weights that do not sum to 1; scores min(count / 3, 1) with zeros among them."""
    rng = np.random.default_rng(seed)
    B, K = dims["B"], dims["K"]
    ids = rng.integers(0, K + 1, (B, G)).astype(np.int32)
    ids[0, :2] = ids[0, 0] if ids[0, 0] > 0 else 1
    ids[1] = 0
    ids[2, 0], ids[3, 0] = 1, K
    w = (rng.integers(1, 8, (B, G)) / 8).astype(np.float32)          # weights on empty entries too: ignored
    cnt = rng.integers(0, 5, (B, G))
    score = np.minimum(cnt.astype(np.float32) / np.float32(3), np.float32(1)).astype(np.float32)
    return ids, w, score


def run_step(m, batch, mode, masks, hop_w, answers=None, labels=True, graph=False):
    if mode == "train":
        m.training()
        m.set_masks(masks)
    else:
        m.evaluate()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"] if labels else None,
                answers=answers)
    if graph:
        m.graph_step(hop_w, zero_grads=True)
    else:
        m.zero_grads()
        m.forward()
    out = {"losses": m.losses(), "logits": m.logits(), "argmax": m.argmax(), "dopred": m.dopred()}
    out["stats"] = m.step_stats()
    if not graph:
        m.backward(hop_w)
    out["grads"] = m.get_grads()
    return out


def assert_same_bits(a, b):
    for k in ("losses", "logits", "argmax", "dopred"):
        assert np.array_equal(a[k], b[k]), k
    for g in a["grads"]:
        assert np.array_equal(a["grads"][g], b["grads"][g]), g
    for k in STAT_KEYS:
        assert np.array_equal(a["stats"][k], b["stats"][k]), k
    assert a["stats"]["did_correct"] == b["stats"]["did_correct"]


# ---------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("dtype,mode,G", [("f32", "train", 1), ("f32", "eval", 1), ("bf16", "train", 1),
                                          ("f32", "train", 16)])
def test_one_unit_entry_gives_the_label_path_bits(dtype, mode, G):
    m, sh, batch, _, masks = make(util.SMALL, dtype=dtype)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    ref = run_step(m, batch, mode, masks, hop_w)
    assert m.batch_answers == 0
    ids = np.zeros((sh.B, G), np.int32)
    ids[:, 0] = batch["labels"]
    w = np.full((sh.B, G), 0.75, np.float32)                          # the empty entries' weights are ignored
    w[:, 0] = 1
    got = run_step(m, batch, mode, masks, hop_w, answers=(ids, w))
    assert m.batch_answers == G
    assert_same_bits(ref, got)
    # a batch without labels that is given a set counts as labelled
    got = run_step(m, batch, mode, masks, hop_w, answers=(ids, w), labels=False)
    assert_same_bits(ref, got)
    # and the next plain batch is back on its labels
    assert_same_bits(ref, run_step(m, batch, mode, masks, hop_w))
    assert m.batch_answers == 0
    m.close()


# ---------------------------------------------------------------- 2. oracle parity by linearity
@functools.lru_cache(maxsize=None)
def expectation(name, mode):
    dims, G, scale = {"small": (util.SMALL, 3, 0.5), "edge": (util.EDGE, 3, 0.5), "medk": (MEDK, 3, 0.2)}[name]
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, seed=123, scale=scale)
    ids, w, _ = answer_set(dims, G, seed=7)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    sh1 = util.shapes(dims, B=1)
    exp = {"losses": np.zeros(sh.H), "g_embed": 0.0, "g_rnn": 0.0, "g_mult": 0.0,
           "logits": np.zeros((sh.H, sh.B, sh.K))}
    for b in range(sh.B):
        m1 = None if mode == "eval" else {k: np.ascontiguousarray(v[:, b:b + 1]) for k, v in masks.items()}
        runs = {}
        for g in range(G):
            y = int(ids[b, g])
            if y == 0:
                continue
            if y not in runs:
                runs[y] = oracle.step(sh1, params, batch["feats"][b:b + 1], batch["tokens"][:, b:b + 1],
                                      batch["lens"][b:b + 1], np.array([y], np.int32), m1, hop_w,
                                      dtype=np.float64)
            r, c = runs[y], float(w[b, g]) / sh.B
            exp["losses"] += c * r["losses"]
            for k in util.GRAD_KEYS:
                exp[k] = exp[k] + c * r[k]
        any_run = next(iter(runs.values()), None)
        if any_run is None:     # a row without entries: forward only
            any_run = oracle.step(sh1, params, batch["feats"][b:b + 1], batch["tokens"][:, b:b + 1],
                                  batch["lens"][b:b + 1], np.array([1], np.int32), m1, hop_w, backward=False,
                                  dtype=np.float64)
        exp["logits"][:, b] = any_run["logits"][:, 0]
    return dims, batch, params, masks, (ids, w), hop_w, exp


@pytest.mark.parametrize("name,mode", [("small", "train"), ("small", "eval"), ("edge", "train"),
                                       ("medk", "train")])
def test_soft_targets_against_the_oracle_by_linearity(name, mode):
    dims, batch, params, masks, answers, hop_w, exp = expectation(name, mode)
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**dims))
    m.set_params(params)
    got = run_step(m, batch, mode, masks, hop_w, answers=answers, labels=False)
    layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
    m.close()
    errs = {"losses": util.rel_err(got["losses"], exp["losses"]),
            "logits": util.rel_err(got["logits"], exp["logits"])}
    for grp in ("embed", "rnn", "mult"):
        for lname, sl in util.layer_slices(layouts[grp]):
            r = exp["g_" + grp][sl]
            if np.max(np.abs(r)) < 1e-12:   # analytically zero (test_gpu_parity's absolute fallback)
                errs[lname] = float(np.max(np.abs(got["grads"][grp][sl] - r)))
            else:
                errs[lname] = util.rel_err(got["grads"][grp][sl], r)
    print(name, mode, {k: f"{v:.2e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"relative errors above {TOL}: {bad}"


# ---------------------------------------------------------------- 3. statistics and scores
def total_ok(tot, rows):
    n = rows.shape[-1]
    r64 = rows.astype(np.float64)
    return np.all(np.abs(tot - r64.sum(-1)) <= (n - 1) * 2.0 ** -24 * np.abs(r64).sum(-1))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_stats_and_scores_match_the_numpy_statement(mode):
    m, sh, batch, _, _ = make(STATS)
    H, B, K = sh.H, sh.B, sh.K
    ids, w, score = answer_set(STATS, 4, seed=3)
    if mode == "train":
        m.training()
        m.set_dropout_seed(11, 2)
    else:
        m.evaluate()
    m.set_batch(**batch, answers=(ids, w, score))
    m.forward()
    s = m.step_stats()
    logits, dopred = m.logits(), m.dopred()
    ref = predict.set_stats(logits, dopred, ids, w, score)
    assert np.array_equal(s["loss"][:H], m.losses())                 # per-hop CE: bitwise rau_get_losses
    print("loss", s["loss"], ref["loss"], "bce", s["loss_do_pred"], ref["loss_do_pred"])
    assert util.rel_err(s["loss"], ref["loss"]) < 1e-4
    assert util.rel_err(s["loss_do_pred"], ref["loss_do_pred"]) < 1e-4
    # counters: exact on the rows a 1e-5 margin decides
    tab = np.stack(predict.merge_hops(logits, dopred, np.zeros((H, B, 1), np.float32))[0][:H + 1])
    _, decided, total = util.argmax_margin_ok(tab.astype(np.float64), ref["ans"][:H + 1], ref["ans"][:H + 1])
    slack = total - decided
    print(f"{decided} of {total} rows decided")
    for k in ("correct", "do_pred_correct"):
        assert np.all(np.abs(s[k] - ref[k]) <= slack), k
    assert abs(s["did_correct"] - ref["did_correct"]) <= slack
    for k in ("fired", "selected"):
        assert np.array_equal(s[k], ref[k]), k
    assert 0 < s["correct"][0] < B                                   # the case decides something
    # scores of the device's own answers
    oe, _ = m.predict()
    per, tot = m.step_scores()
    fired = (dopred > 0.5).any(0)
    ans = oe.copy()
    ans[H + 1] = np.where(fired, oe[H + 1], 1)                       # feval: no hop fired -> the all-zero row's answer 1
    assert np.array_equal(m.argmax(), oe[:H])
    want = predict.answer_score(ans, ids, score)
    assert per.dtype == np.float32 and np.array_equal(per, want)
    assert total_ok(tot, per)
    per2, tot2 = m.step_scores()
    assert np.array_equal(per, per2) and np.array_equal(tot, tot2)
    s2 = m.step_stats()
    for k in STAT_KEYS:
        assert np.array_equal(s[k], s2[k]), k
    # predict_scores: open-ended only, then with an MC list
    po, pm, pt = m.predict_scores(mc=True)
    assert np.array_equal(po, predict.answer_score(oe, ids, score)) and not pm.any() and not pt[1].any()
    assert total_ok(pt[0], po)
    rng = np.random.default_rng(2)
    mc_list = rng.integers(0, K + 1, (B, 5)).astype(np.int32)
    oe2, mc2 = m.predict(mc_list)
    po2, pm2, pt2 = m.predict_scores(mc=True)
    assert np.array_equal(oe2, oe) and np.array_equal(po2, po)
    assert np.array_equal(pm2, predict.answer_score(mc2, ids, score))
    assert total_ok(pt2[0], po2) and total_ok(pt2[1], pm2)
    again = m.predict_scores(mc=True)
    assert all(np.array_equal(a, b) for a, b in zip((po2, pm2, pt2), again))
    # weights as scores when no score is given
    m.set_answers(ids, w)
    m.forward()
    assert np.array_equal(m.step_scores()[0][:H], predict.answer_score(m.argmax(), ids, w))
    m.close()


# ---------------------------------------------------------------- 4. state
def rc_scores(m):
    return (m._lib.rau_step_scores(m._h, None, None), m._lib.rau_predict_scores(m._h, None, None, None))


def rc_set(m, ids, w, score=None, slot=-1, G=None):
    return m._lib.rau_set_answers(m._h, slot, ids.shape[1] if G is None else G, ids.ctypes.data, w.ctypes.data,
                                  None if score is None else score.ctypes.data)


def test_lifetime_errors_and_the_two_slots():
    m, sh, batch, _, _ = make(util.SMALL)
    ids, w, score = answer_set(util.SMALL, 3, seed=1)
    m.evaluate()
    assert rc_set(m, ids, w) == STATE                                # no batch yet
    m.set_batch(**batch)
    m.forward()
    m.predict()
    assert rc_scores(m) == (STATE, STATE)                            # no set
    m.set_answers(ids, w, score)
    assert m.batch_answers == 3
    assert m._lib.rau_step_stats(m._h, None, None, None) == STATE    # the forward read the labels: run it again
    m.forward()
    assert m._lib.rau_predict_scores(m._h, None, None, None) == STATE   # no rau_predict on THIS forward
    m.predict()
    good = m.step_scores()[0]
    # invalid sets leave the previous one in force
    bad_id, bad_w, bad_s = ids.copy(), w.copy(), score.copy()
    bad_id[4, 1] = sh.K + 1
    bad_w[2, 2] = -0.5
    bad_s[0, 0] = np.inf
    wide = np.ones((sh.B, 17), np.int32)
    for rc in (rc_set(m, bad_id, w), rc_set(m, -bad_id, w), rc_set(m, ids, bad_w), rc_set(m, ids, w, bad_s),
               rc_set(m, ids, w * np.float32("nan")), rc_set(m, ids, w, G=0),
               rc_set(m, wide, wide.astype(np.float32))):
        assert rc == INVALID
    assert m._lib.rau_set_answers(m._h, 2, 3, ids.ctypes.data, w.ctypes.data, None) == INVALID
    assert m.batch_answers == 3 and np.array_equal(m.step_scores()[0], good)
    # an upload into the slot clears the set; so does set_batch_size
    m.set_batch(**batch)
    assert m.batch_answers == 0
    m.forward()
    assert rc_scores(m)[0] == STATE
    m.set_answers(ids, w, score)
    m.set_batch_size(sh.B - 1)
    assert m.batch_answers == 0
    m.set_batch_size(sh.B)
    # asynchronous path == synchronous path, and the set survives an upload into the other slot
    m.set_batch(**batch, answers=(ids, w, score))
    m.forward()
    m.predict()
    sync = (m.losses(), m.step_stats(), m.step_scores(), m.predict_scores())
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], None, has_labels=False,
                      answers=(ids, w, score))
    m.use_batch(1)
    m.set_batch_async(0, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])   # the other slot
    assert m.batch_answers == 3
    m.forward()
    m.predict()
    assert np.array_equal(m.losses(), sync[0])
    st = m.step_stats()
    for k in STAT_KEYS:
        assert np.array_equal(st[k], sync[1][k]), k
    for a, b in zip(m.step_scores() + m.predict_scores()[::2], sync[2] + sync[3][::2]):
        assert np.array_equal(a, b)
    m.use_batch(0)                                                   # a batch without a set
    assert m.batch_answers == 0
    m.forward()
    assert rc_scores(m)[0] == STATE
    m.use_batch(1)                                                   # slot 1 still holds its set
    assert m.batch_answers == 3
    m.forward()
    assert np.array_equal(m.step_scores()[0], sync[2][0])
    assert rc_set(m, ids, w, slot=1) == STATE                        # current batch of an unfinished forward
    m.close()


def test_image_table_and_bank_batches_take_a_set():
    m, sh, batch, _, _ = make(util.SMALL)
    ids, w, score = answer_set(util.SMALL, 2, seed=4)
    m.evaluate()
    m.set_batch(**batch, answers=(ids, w, score))
    m.forward()
    ref = (m.losses(), m.step_scores()[0])
    image_of = np.arange(sh.B, dtype=np.int32)[::-1].copy()
    table = np.ascontiguousarray(batch["feats"][::-1])
    m.set_batch(table, batch["tokens"], batch["lens"], None, image_of=image_of, answers=(ids, w, score))
    m.forward()
    assert m.batch_images() == sh.B and m.batch_answers == 2
    assert np.array_equal(m.losses(), ref[0]) and np.array_equal(m.step_scores()[0], ref[1])
    m.bank_create(sh.B)
    m.bank_put(0, table)
    m.set_batch(None, batch["tokens"], batch["lens"], None, bank_rows=np.arange(sh.B), image_of=image_of,
                answers=(ids, w, score))
    m.forward()
    assert np.array_equal(m.losses(), ref[0]) and np.array_equal(m.step_scores()[0], ref[1])
    m.close()


# ---------------------------------------------------------------- 5. graph
def test_graph_step_with_a_set_gives_the_eager_bits():
    m, sh, batch, _, masks = make(util.SMALL)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    ids, w, score = answer_set(util.SMALL, 3, seed=5)
    ids2, w2, _ = answer_set(util.SMALL, 5, seed=6)
    eager = run_step(m, batch, "train", masks, hop_w, answers=(ids, w, score))
    eager2 = run_step(m, batch, "train", masks, hop_w, answers=(ids2, w2))
    eager0 = run_step(m, batch, "train", masks, hop_w)
    # captured without a set first: a batch with one must not replay that graph, nor one of another G
    assert_same_bits(eager0, run_step(m, batch, "train", masks, hop_w, graph=True))
    assert_same_bits(eager, run_step(m, batch, "train", masks, hop_w, answers=(ids, w, score), graph=True))
    assert_same_bits(eager2, run_step(m, batch, "train", masks, hop_w, answers=(ids2, w2), graph=True))
    assert_same_bits(eager, run_step(m, batch, "train", masks, hop_w, answers=(ids, w, score), graph=True))   # replay
    assert_same_bits(eager0, run_step(m, batch, "train", masks, hop_w, graph=True))
    assert not np.array_equal(eager["losses"], eager0["losses"])
    m.close()


# ---------------------------------------------------------------- 6. module level
def test_criterion_set_modules_equal_the_step():
    m, sh, batch, _, _ = make(util.SMALL)
    H, B, K = sh.H, sh.B, sh.K
    ids, w, _ = answer_set(util.SMALL, 3, seed=8)
    m.evaluate()
    m.set_batch(**batch, answers=(ids, w))
    m.forward()
    losses, logits = m.losses(), m.logits()
    lib, h = m._lib, m._h

    def dev(a):
        p = C.c_void_p()
        L.check(lib.rau_dev_alloc(h, a.size, C.byref(p)))
        L.check(lib.rau_dev_upload(h, p, a.ctypes.data, a.nbytes))
        return p

    def down(ptr):
        out = np.empty((B, K), np.float32)
        L.check(lib.rau_dev_download(h, out.ctypes.data, C.c_void_p(ptr), out.nbytes))
        return out
    ids_d, w_d = dev(ids), dev(w)
    lg_d = [dev(np.ascontiguousarray(logits[k])) for k in range(H)]
    # the step's own dl slots: criterion h writes the slot the step's head wrote for hop h, so the pointer of
    # the last hop's slot (taken first) locates the others before they are overwritten
    p = C.c_void_p()
    L.check(lib.rau_criterion_backward_set(h, H - 1, lg_d[H - 1], 3, ids_d, w_d, 1.0, C.byref(p)))
    step_dl = [down(p.value - (H - 1 - k) * B * K * 4) for k in range(H - 1)]
    for k in range(H - 1):
        loss = C.c_float()
        L.check(lib.rau_criterion_forward_set(h, k, lg_d[k], 3, ids_d, w_d, C.byref(loss)))
        assert np.float32(loss.value) == losses[k]
        q = C.c_void_p()
        L.check(lib.rau_criterion_backward_set(h, k, lg_d[k], 3, ids_d, w_d, 1.0, C.byref(q)))
        assert q.value == p.value - (H - 1 - k) * B * K * 4
        dl = down(q.value)
        assert np.array_equal(dl, step_dl[k])
        assert util.rel_err(dl, predict.soft_ce_grad(logits[k], ids, w)) < 1e-5
        L.check(lib.rau_criterion_backward_set(h, k, lg_d[k], 3, ids_d, w_d, 2.0, C.byref(q)))
        assert np.array_equal(down(q.value), dl * np.float32(2))
        # labels_dev == NULL: the resident batch's set
        L.check(lib.rau_criterion_backward(h, k, lg_d[k], None, 1.0, C.byref(q)))
        assert np.array_equal(down(q.value), dl)
        L.check(lib.rau_criterion_forward(h, k, lg_d[k], None, C.byref(loss)))
        assert np.float32(loss.value) == losses[k]
    assert lib.rau_criterion_forward_set(h, 0, lg_d[0], 17, ids_d, w_d, None) == INVALID
    m.close()
