"""rau_step_stats / rau_predict / rau_get_merged (hop_merge.hip): feval's joint-loss statistics
and predict_result's merged answers on the device, against the host restatements
(joint.feval_stats, predict.merge_hops / answers / predict_result)."""
import ctypes as C

import numpy as np
import pytest

from rau_vqa_amd import joint, predict, synth
from rau_vqa_amd import _lib as L
from tests import util

pytestmark = pytest.mark.gpu

DIMS = dict(B=37, T=6, V=50, E=8, Rq=16, D=24, S=49, M=40, A=20, R=16, K=12, H=3)
COUNT_KEYS = ("correct", "do_pred_correct", "fired", "selected")
STATE, INVALID = -3, -1


def make(dims, dtype="f32", seed=123, scale=0.5):
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(dims)
    batch, params, masks = util.make_problem(sh, seed=seed, scale=scale)
    m = RAU(Config(**dims, dtype=dtype))
    m.set_params(params)
    return m, batch, params, masks


def set_param(m, params, name, value):
    off = {n: o for n, o, _, _ in m.layout("mult")}[name]
    p = {k: v.copy() for k, v in params.items()}
    p["mult"][off] = value
    m.set_params(p)


def rc_stats(m):
    return m._lib.rau_step_stats(m._h, None, None, None)


def rel_ok(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.abs(b)))


def check_against_host(m, labels):
    """device stats == feval_stats on the device's own downloaded outputs"""
    s = m.step_stats()
    ref = joint.feval_stats(m.logits(), m.dopred(), labels)
    H = m.cfg.H
    assert np.array_equal(s["loss"][:H], m.losses())          # bitwise the step's own losses
    assert rel_ok(s["loss"], ref["loss"], 2e-6), (s["loss"], ref["loss"])
    assert rel_ok(s["loss_do_pred"], ref["loss_do_pred"], 2e-6)
    for k in COUNT_KEYS:
        assert np.array_equal(s[k], ref[k]), k
    assert s["did_correct"] == ref["did_correct"]
    return s


def test_fixtures_against_oracle_outputs():
    from tests.test_golden import FIXTURES, load
    from rau_vqa_amd.model import RAU, Config
    for path in FIXTURES:
        sh, batch, params, masks, train, _, z = load(path)
        m = RAU(Config(**{k: getattr(sh, k) for k in
                          ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H",
                           "p_we", "p_rnn", "p_q", "p_x", "p_mf")}))
        m.set_params(params)
        if train:
            m.training()
            m.set_masks(masks)
        else:
            m.evaluate()
        m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
        m.forward()
        s, argmax = m.step_stats(), m.argmax()
        m.close()
        ref = joint.feval_stats(z["o_logits"], z["o_dopred"], batch["labels"])
        assert util.rel_err(s["loss"], ref["loss"]) < 1e-4, path
        assert util.rel_err(s["loss_do_pred"], ref["loss_do_pred"]) < 1e-4, path
        # counts wherever the fp64 reference decides every answer and every do_pred threshold
        uni = z["o_logits"].mean(0)
        _, dec_h, tot_h = util.argmax_margin_ok(z["o_logits"], argmax, z["o_argmax"])
        _, dec_u, tot_u = util.argmax_margin_ok(uni, ref["uni_ans"], ref["uni_ans"])
        if dec_h == tot_h and dec_u == tot_u and np.all(np.abs(z["o_dopred"] - 0.5) > 1e-5):
            for k in COUNT_KEYS:
                assert np.array_equal(s[k], ref[k]), (path, k)
            assert s["did_correct"] == ref["did_correct"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_device_stats_match_host_restatement(dtype, mode):
    m, batch, _, _ = make(DIMS, dtype=dtype)
    if mode == "train":
        m.training()
        m.set_dropout_seed(11, 2)      # Philox masks
    else:
        m.evaluate()
    m.set_batch(**batch)
    m.forward()
    s1 = check_against_host(m, batch["labels"])
    s2 = m.step_stats()                # repeated queries: the same bits
    for k in ("loss", "loss_do_pred") + COUNT_KEYS:
        assert np.array_equal(s1[k], s2[k])
    m.close()


def test_device_stats_at_the_benchmark_shape():
    from rau_vqa_amd.model import RAU, Config
    cfg = Config(B=256)                # configs[1]: Ours_SS, 14x14x512, 8 hops, K = 1000
    m = RAU(cfg)
    m.init_uniform(5, -0.08, 0.08)
    batch = synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=5)
    m.training()
    m.set_dropout_seed(3, 1)
    m.set_batch(**batch)
    m.forward()
    check_against_host(m, batch["labels"])
    m.close()


def test_do_pred_bias_all_fire_and_none_fire():
    m, batch, params, _ = make(DIMS)
    m.evaluate()
    B, H, K = DIMS["B"], DIMS["H"], DIMS["K"]
    set_param(m, params, "classifier.out_do_pred.bias", 30.0)
    m.set_batch(**batch)
    m.forward()
    s = check_against_host(m, batch["labels"])
    assert list(s["fired"]) == [B] * H and list(s["selected"]) == [B] + [0] * (H - 1)
    assert s["loss"][H + 1] == s["loss"][0]          # select row == hop 1, bitwise its CE
    assert s["correct"][H + 1] == s["correct"][0]
    set_param(m, params, "classifier.out_do_pred.bias", -30.0)
    m.forward()
    s = check_against_host(m, batch["labels"])
    assert not s["fired"].any() and not s["selected"].any()
    assert s["loss"][H + 1] == pytest.approx(np.log(K), rel=1e-6)
    assert s["correct"][H + 1] == int((batch["labels"] == 1).sum())   # all-zero row: answer 1
    m.close()


def test_stats_survive_backward_and_graph_step_and_change_nothing():
    dims = dict(util.SMALL)
    hop_w = np.full(dims["H"], float(dims["H"]), np.float32)
    runs = []
    for query in (True, False):
        m, batch, _, _ = make(dims, seed=9)
        m.training()
        m.set_dropout_seed(4, 0)
        m.set_batch(**batch)
        m.zero_grads()
        m.forward()
        got = [m.step_stats()] if query else []
        m.backward(hop_w)
        if query:
            got.append(m.step_stats())
        out = [m.logits(), m.get_grads()]
        m.graph_step(hop_w, zero_grads=True)
        if query:
            got.append(m.step_stats())
        out += [m.logits(), m.get_grads()]
        m.close()
        runs.append(out)
        for s in got[1:]:
            for k in ("loss", "loss_do_pred") + COUNT_KEYS:
                assert np.array_equal(s[k], got[0][k]), k
    for a, b in zip(runs[0], runs[1]):
        if isinstance(a, dict):
            for g in a:
                assert np.array_equal(a[g], b[g]), g
        else:
            assert np.array_equal(a, b)


def test_state_errors_and_the_other_slot():
    m, batch, _, _ = make(DIMS)
    B, Q = DIMS["B"], 4 * DIMS["Rq"]
    hop_w = np.ones(DIMS["H"], np.float32)
    assert rc_stats(m) == STATE                                   # no forward yet
    assert m._lib.rau_predict(m._h, None, 0, None, None) == STATE
    assert m._lib.rau_get_merged(m._h, None, None) == STATE
    m.evaluate()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], None)
    m.forward()
    assert rc_stats(m) == STATE                                   # no labels
    m.predict()                                                   # predict needs none
    m.set_batch(**batch)
    m.forward()
    s0 = m.step_stats()
    m.set_batch(**batch)
    assert rc_stats(m) == STATE                                   # the same slot rewritten
    m.forward()
    q = C.c_void_p()
    L.check(m._lib.rau_dev_alloc(m._h, B * Q, C.byref(q)))
    outs = [C.c_void_p() for _ in range(5)]
    L.check(m._lib.rau_multimodal_forward(m._h, 0, q, None, None, None, *[C.byref(o) for o in outs]))
    assert rc_stats(m) == STATE                                   # module-level call since
    # asynchronous slots: an upload into the other slot keeps the stats
    m.training()
    m.set_batch_async(0, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.use_batch(0)
    m.evaluate()
    m.forward()
    s1 = m.step_stats()
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    s2 = m.step_stats()
    for k in ("loss",) + COUNT_KEYS:
        assert np.array_equal(s0[k], s1[k]) and np.array_equal(s1[k], s2[k])
    m.backward(hop_w)
    m.step_stats()
    m.set_batch_async(0, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    assert rc_stats(m) == STATE                                   # its own slot refilled
    m.close()


def mc_lists(rng, B, K, n=6):
    mc = rng.integers(0, K + 1, size=(B, n)).astype(np.int32)
    mc[:, 1] = 0                      # empty slots
    mc[:, 3] = mc[:, 2]               # duplicates
    mc[0] = 0                         # no candidate at all
    mc[1] = np.minimum(np.arange(1, n + 1), K)
    return mc


@pytest.mark.parametrize("dims", [DIMS, dict(util.EDGE)], ids=["H3", "H1"])
def test_predict_matches_host_merges_and_answers(dims):
    m, batch, params, _ = make(dims, seed=21)
    rng = np.random.default_rng(2)
    B, K = dims["B"], dims["K"]
    m.evaluate()
    for bias in (None, -50.0):        # -50: every logit negative, the MC quirk decides
        if bias is not None:
            off = {n: o for n, o, _, _ in m.layout("mult")}["classifier.out_score.bias"]
            p = {k: v.copy() for k, v in params.items()}
            p["mult"][off:off + K] = bias
            m.set_params(p)
        mc = mc_lists(rng, B, K)
        host = predict.predict_result(m, batch["feats"], batch["tokens"], batch["lens"], mc)
        dev = predict.predict_result_device(m, batch["feats"], batch["tokens"], batch["lens"], mc)
        assert np.array_equal(dev["oe"], host["oe"]) and np.array_equal(dev["mc"], host["mc"])
        for a, b in zip(dev["tab_pred"] + dev["tab_att"], host["tab_pred"] + host["tab_att"]):
            assert np.array_equal(a, b)
        # the carried select attention map over a second batch
        host2 = predict.predict_result(m, batch["feats"], batch["tokens"], batch["lens"], mc,
                                       select_att_state=host["tab_att"][-1])
        dev2 = predict.predict_result_device(m, batch["feats"], batch["tokens"], batch["lens"], mc,
                                             select_att_state=dev["tab_att"][-1])
        assert np.array_equal(dev2["tab_att"][-1], host2["tab_att"][-1])
        oe, mcs = m.predict(None)
        assert mcs is None and np.array_equal(oe, host["oe"])
        if bias is not None:
            assert np.all(dev["tab_pred"][0] < 0) and np.all(dev["mc"][:, 0] == 1)
    bad = mc_lists(rng, B, K)
    bad[2, 0] = K + 1
    assert m._lib.rau_predict(m._h, bad.ctypes.data, bad.shape[1], None, None) == INVALID
    bad[2, 0] = -1
    assert m._lib.rau_predict(m._h, bad.ctypes.data, bad.shape[1], None, None) == INVALID
    m.close()
