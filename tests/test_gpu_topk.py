"""rau_dev_topk / rau_topk (topk.hip): ranked answers with scores and softmax confidences on the
device, against the numpy statement of the contract (predict.top_answers, pinned by
tests/test_topk_host.py).  Ids and scores are compared EXACTLY: both sides order the same f32 bits."""
import ctypes as C
import math

import numpy as np
import pytest

from rau_vqa_amd import predict
from rau_vqa_amd import _lib as L
from tests import util

pytestmark = pytest.mark.gpu

DIMS = dict(B=37, T=6, V=50, E=8, Rq=16, D=24, S=49, M=40, A=20, R=16, K=12, H=3)   # test_gpu_hop_merge.DIMS
WIDE = dict(B=5, T=6, V=50, E=8, Rq=16, D=24, S=49, M=40, A=20, R=16, K=1000, H=2)  # the real answer width
STATE, INVALID = -3, -1
# The issue's shapes, and one pair either side of the LDS staging budget of topk.hip (4096 floats):
# (2, 5000, 4) already runs the global re-read path, these two pin the threshold itself.
SHAPES = [(5, 12, 3), (3, 1, 1), (4, 63, 63), (4, 64, 7), (4, 65, 65), (3, 257, 9), (2, 1003, 10),
          (2, 5000, 4), (2, 4096, 3), (2, 4097, 3)]
KINDS = ("gauss", "ties", "equal", "special", "nan")
U_EXP = 1   # ulp bound of device expf in the HIP math API documentation's accuracy table


def make(dims, dtype="f32", seed=123, scale=0.5):
    from rau_vqa_amd.model import RAU, Config
    batch, params, _ = util.make_problem(util.shapes(dims), seed=seed, scale=scale)
    m = RAU(Config(**dims, dtype=dtype))
    m.set_params(params)
    return m, batch, params


def set_param(m, params, name, value):
    off = {n: o for n, o, _, _ in m.layout("mult")}[name]
    p = {k: v.copy() for k, v in params.items()}
    p["mult"][off] = value
    m.set_params(p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def crafted(kind, rows, cols, rng):
    if kind == "gauss":
        return rng.standard_normal((rows, cols)).astype(np.float32)
    if kind == "ties":
        return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=(rows, cols))
    if kind == "equal":
        return np.full((rows, cols), np.float32(rng.standard_normal()), np.float32)
    if kind == "nan":
        x = np.full((rows, cols), np.nan, np.float32)
        x.view(np.uint32)[:, ::2] |= np.uint32(0x80000005)     # signs and payloads differ
        return x
    x = rng.standard_normal((rows, cols)).astype(np.float32)   # special: +inf, -inf, three NaNs per row
    special = np.array([np.inf, -np.inf, np.nan, np.nan, np.nan], np.float32)
    for r in range(rows):
        n = min(cols, 5)
        x[r, rng.choice(cols, n, replace=False)] = np.roll(special, r)[:n]
    return x


class Dev:
    """a small context and three device buffers for the rau_dev_* calls"""

    def __init__(self):
        self.m, _, _ = make(dict(util.EDGE))
        self.lib, self.h = self.m._lib, self.m._h
        self.x, self.v, self.i = (self.alloc(n) for n in (10240, 1024, 1024))

    def alloc(self, n):
        p = C.c_void_p()
        L.check(self.lib.rau_dev_alloc(self.h, n, C.byref(p)))
        return p

    def topk(self, x, k, want_val=True, want_idx=True):
        rows, cols = x.shape
        assert x.size <= 10240 and rows * k <= 1024                 # the buffers above
        L.check(self.lib.rau_dev_upload(self.h, self.x, x.ctypes.data, x.nbytes))
        for buf in (self.v, self.i):
            L.check(self.lib.rau_dev_fill(self.h, buf, 1024, -7.0))
        L.check(self.lib.rau_dev_topk(self.h, self.x, rows, cols, k, self.v if want_val else None,
                                      self.i if want_idx else None))
        val, idx = np.empty((rows, k), np.float32), np.empty((rows, k), np.int32)
        L.check(self.lib.rau_dev_download(self.h, val.ctypes.data, self.v, val.nbytes))
        L.check(self.lib.rau_dev_download(self.h, idx.ctypes.data, self.i, idx.nbytes))
        return val, idx

    def rowmax(self, x):
        rows, cols = x.shape
        L.check(self.lib.rau_dev_upload(self.h, self.x, x.ctypes.data, x.nbytes))
        L.check(self.lib.rau_dev_rowmax(self.h, self.x, rows, cols, self.v, self.i))
        val, idx = np.empty(rows, np.float32), np.empty(rows, np.int32)
        L.check(self.lib.rau_dev_download(self.h, val.ctypes.data, self.v, val.nbytes))
        L.check(self.lib.rau_dev_download(self.h, idx.ctypes.data, self.i, idx.nbytes))
        return val, idx


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.m.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dev_topk_on_crafted_matrices(dev, shape):
    rows, cols, k = shape
    rng = np.random.default_rng(rows * 100003 + cols)
    untouched = bits(np.full((rows, k), -7.0, np.float32))
    for kind in KINDS:
        x = crafted(kind, rows, cols, rng)
        ids, score, _ = predict.top_answers(x[None], k)
        val, idx = dev.topk(x, k)
        assert np.array_equal(idx, ids[0]), kind
        assert np.array_equal(bits(val), bits(score[0])), kind
        assert np.all((idx >= 1) & (idx <= cols)), kind
        assert all(len(set(r)) == k for r in idx.tolist()), kind
        val2, idx2 = dev.topk(x, k)                                  # repeated calls: the same bits
        assert np.array_equal(bits(val2), bits(val)) and np.array_equal(idx2, idx), kind
        v_only, i_none = dev.topk(x, k, want_idx=False)              # the NULL-output forms
        assert np.array_equal(bits(v_only), bits(val)) and np.array_equal(bits(i_none.view(np.float32)), untouched)
        v_none, i_only = dev.topk(x, k, want_val=False)
        assert np.array_equal(i_only, idx) and np.array_equal(bits(v_none), untouched), kind
        if kind in ("gauss", "ties", "equal"):                       # NaN-free: rank 0 is rau_dev_rowmax
            mv, mi = dev.rowmax(x)
            assert np.array_equal(mi, idx[:, 0]) and np.array_equal(bits(mv), bits(val[:, 0])), kind


def test_dev_topk_argument_rules(dev):
    lib, h = dev.lib, dev.h
    assert lib.rau_dev_topk(h, dev.x, 0, 7, 3, dev.v, dev.i) == 0    # no rows: a no-op
    for rows, cols, k in ((-1, 7, 3), (2, 0, 1), (2, 7, 0), (2, 7, 8)):
        assert lib.rau_dev_topk(h, dev.x, rows, cols, k, dev.v, dev.i) == INVALID
    assert lib.rau_dev_topk(h, None, 2, 7, 3, dev.v, dev.i) == INVALID
    x = np.arange(14, dtype=np.float32).reshape(2, 7)
    val, idx = dev.topk(x, 7)                                        # a valid call straight after
    assert idx.tolist() == [[7, 6, 5, 4, 3, 2, 1]] * 2
    # the device-tensor method
    from rau_vqa_amd.modules import DevTensor
    t = DevTensor.zeros(dev.m, 2, 7).copy(x)
    v, i = t.topk(3)
    assert i.numpy("int32").tolist() == [[7, 6, 5]] * 2 and np.array_equal(v.numpy(), x[:, :3:-1])


def conf_bound(K, spread):
    """Relative bound on conf = fdiv(expf(score - mx), den) against the float64 softmax, in units of
    2^-24: 2 u_exp (the numerator's expf and the summands'), ceil(K / 256) (each thread's running sum),
    8 (the 6-level wave tree and the two adds across waves), 1 (the division), 2 spread (the rounding
    of v - mx, up to 2^-24 |v - mx|, scales expf's result by that much, in the numerator and in the
    dominant summands)."""
    return (2 * U_EXP + math.ceil(K / 256) + 8 + 1 + 2 * spread) * 2.0 ** -24


def check_topk(m, k, tag=""):
    """device rau_topk == merge_hops on the downloaded outputs, then top_answers"""
    tab_pred, _ = predict.merge_hops(m.logits(), m.dopred(), m.attention())
    rid, rscore, _ = predict.top_answers(tab_pred, k)
    ids, score, conf = m.topk(k)
    H, K = m.cfg.H, m.cfg.K
    assert ids.shape == rid.shape == (H + 2, tab_pred[0].shape[0], k)
    assert ids.dtype == np.int32 and score.dtype == np.float32 and conf.dtype == np.float32
    assert np.array_equal(ids, rid), tag
    assert np.array_equal(bits(score), bits(rscore)), tag
    assert np.array_equal(ids[..., 0], m.predict()[0]), tag
    x = np.stack(tab_pred).astype(np.float64)
    mx = x.max(-1, keepdims=True)
    soft = np.exp(rscore.astype(np.float64) - mx) / np.exp(x - mx).sum(-1, keepdims=True)
    spread = float(np.max(mx - rscore))
    err = np.abs(conf.astype(np.float64) - soft) / soft
    bound = conf_bound(K, spread)
    print(f"topk conf {tag} K={K} k={k} spread={spread:.3f} max_rel_err={err.max():.3e} "
          f"bound={bound:.3e} ratio={err.max() / bound:.3f}")
    assert np.all(err <= bound), (tag, float(err.max()), bound)
    return ids, score, conf


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_topk_matches_host_restatement(dtype):
    m, batch, _ = make(DIMS, dtype=dtype)
    m.evaluate()
    m.set_batch(**batch)
    m.forward()
    for k in (1, 5, 12):
        a = check_topk(m, k, dtype)
        b = m.topk(k)                                                # repeated queries: the same bits
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    m.close()


def test_topk_select_row_with_do_pred_forced_high_and_low():
    m, batch, params = make(DIMS)
    m.evaluate()
    H = DIMS["H"]
    m.set_batch(**batch)
    for bias, hop in ((30.0, 0), (-30.0, H - 1)):                   # every hop fires / none does: the last is forced
        set_param(m, params, "classifier.out_do_pred.bias", bias)
        m.forward()
        for k in (1, 5, 12):
            ids, score, conf = check_topk(m, k, f"bias{bias:+.0f}")
            assert np.array_equal(ids[H + 1], ids[hop])
            # select = 0 + l_hop: the same value (a -0 logit becomes +0)
            assert np.array_equal(score[H + 1], score[hop])
    m.close()


def test_topk_at_the_real_answer_width():
    m, batch, _ = make(WIDE, seed=31)
    m.evaluate()
    m.set_batch(**batch)
    m.forward()
    check_topk(m, 10, "K1000")
    res = predict.predict_result_device(m, batch["feats"], batch["tokens"], batch["lens"], tabs=False, topk=10)
    ids, score, conf = m.topk(10)
    assert np.array_equal(res["top_ids"], ids) and np.array_equal(res["top_score"], score)
    assert np.array_equal(res["top_conf"], conf)
    plain = predict.predict_result_device(m, batch["feats"], batch["tokens"], batch["lens"], tabs=False)
    assert sorted(plain) == ["mc", "oe", "tab_att", "tab_pred"]      # the default result is unchanged
    m.close()


def test_topk_state_and_argument_errors():
    m, batch, _ = make(DIMS)
    B, K, Q = DIMS["B"], DIMS["K"], 4 * DIMS["Rq"]
    rc = lambda k: m._lib.rau_topk(m._h, k, None, None, None)
    assert rc(1) == STATE                                            # no forward yet
    m.evaluate()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], None)   # needs no labels
    m.forward()
    assert rc(0) == INVALID and rc(K + 1) == INVALID and rc(-3) == INVALID
    check_topk(m, 3)                                                 # a valid call straight after
    m.set_batch(**batch)
    assert rc(1) == STATE                                            # the slot that forward read was rewritten
    m.forward()
    assert rc(K) == 0
    q = C.c_void_p()
    L.check(m._lib.rau_dev_alloc(m._h, B * Q, C.byref(q)))
    outs = [C.c_void_p() for _ in range(5)]
    L.check(m._lib.rau_multimodal_forward(m._h, 0, q, None, None, None, *[C.byref(o) for o in outs]))
    assert rc(1) == STATE                                            # module-level call since
    m.forward()
    check_topk(m, 2)
    m.close()


def test_topk_between_forward_and_backward_changes_nothing_and_follows_graph_step():
    dims = dict(util.SMALL)
    hop_w = np.full(dims["H"], float(dims["H"]), np.float32)
    runs = []
    for query in (True, False):
        m, batch, _ = make(dims, seed=9)
        m.training()
        m.set_dropout_seed(4, 0)                                     # a train-mode forward with Philox masks
        m.set_batch(**batch)
        m.zero_grads()
        m.forward()
        if query:
            first = check_topk(m, 5, "train")
            stats, oe = m.step_stats(), m.predict()[0]
        m.backward(hop_w)
        if query:                                                    # still valid, the same bits; nothing disturbed
            for u, v in zip(first, m.topk(5)):
                assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
            assert np.array_equal(m.step_stats()["loss"], stats["loss"]) and np.array_equal(m.predict()[0], oe)
        out = [m.logits(), m.get_grads()]
        m.graph_step(hop_w, zero_grads=True)
        if query:
            check_topk(m, 5, "graph")
        out += [m.logits(), m.get_grads()]
        m.close()
        runs.append(out)
    for a, b in zip(runs[0], runs[1]):
        if isinstance(a, dict):
            assert sorted(a) == ["embed", "mult", "rnn"]
            for g in a:
                assert np.array_equal(a[g], b[g]), g
        else:
            assert np.array_equal(a, b)


def test_topk_grows_k_and_follows_set_batch_size():
    m, batch, _ = make(DIMS)
    m.evaluate()
    m.set_batch(**batch)
    m.forward()
    check_topk(m, 1, "k1")
    check_topk(m, 12, "grown")                                       # the staging is regrown
    check_topk(m, 4, "shrunk")
    n = 23
    small, _, _ = util.make_problem(util.shapes(DIMS, B=n), seed=5, scale=0.5)
    m.set_batch_size(n)
    assert m._lib.rau_topk(m._h, 1, None, None, None) == STATE       # the results did not outlive the resize
    m.set_batch(**small)
    m.forward()
    ids, _, _ = check_topk(m, 12, "n23")
    assert ids.shape == (DIMS["H"] + 2, n, 12)
    m.close()
