"""Per-sample loss weights (rau_set_sample_weights) on the host: the numpy statements of rau_vqa_amd/joint.py and
predict.py with weights, against torch fp64 autograd of the objective they state,

    (1/n) sum_b s_b row_b        for every built-in mean (1/n) sum_b row_b,

RAU.set_sample_weights' argument checks and its normalize=, and the all-ones identity.  No GPU, no library call.
"""
import numpy as np
import pytest
import torch

from rau_vqa_amd import joint, predict
from rau_vqa_amd.model import RAU

H, B, K, S, G = 3, 8, 12, 12, 3
EPS = 1e-12


def weights(seed=1, n=B):
    """Uniform in [0, 2] with one exact zero."""
    s = np.random.default_rng(seed).uniform(0, 2, size=n).astype(np.float32)
    s[3 % n] = 0.0
    return s


def problem(seed=0):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(H, B, K)).astype(np.float32) * 2
    dopred = rng.uniform(0.05, 0.95, size=(H, B)).astype(np.float32)
    labels = rng.integers(1, K + 1, size=B).astype(np.int32)
    ids = rng.integers(1, K + 1, size=(B, G)).astype(np.int32)
    ids[1] = 0                     # a row without entries
    ids[4, 1] = 0
    ids[3, 2] = ids[3, 0]          # a duplicate
    w = rng.uniform(0.1, 1.0, size=(B, G)).astype(np.float32)
    att = rng.uniform(0.01, 1, size=(H, B, S))
    att = (att / att.sum(-1, keepdims=True)).astype(np.float32)
    t = rng.uniform(0, 1, size=(B, S)).astype(np.float32)
    t[2] = 0                       # an unsupervised row
    t[t < 0.3] = 0
    nreg = np.array([12, 7, 3, 1, 5, 12, 2, 9], np.int32)
    return logits, dopred, labels, ids, w, att, t, nreg


def t64(a, grad=False):
    return torch.as_tensor(np.asarray(a, np.float64)).clone().requires_grad_(grad)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / max(np.max(np.abs(b)), 1e-30))


# ------------------------------------------------------------------------------------------ 1. against autograd
def test_weighted_mean_of_the_ce_rows_and_its_gradient():
    logits, _dp, labels, _ids, _w, _a, _t, _n = problem()
    s = weights()
    x = t64(logits[0], True)
    rows = torch.nn.functional.cross_entropy(x, torch.as_tensor(labels).long() - 1, reduction="none")
    obj = (t64(s) * rows).sum() / B
    obj.backward()
    got_rows = predict.soft_ce(logits[0], labels[:, None], np.ones((B, 1), np.float32))[0]
    assert rel(joint.weighted_mean(got_rows, s), obj.item()) < 1e-6
    assert rel(joint.cross_entropy(logits[0], labels.astype(np.int64), s), obj.item()) < 1e-6
    g = s[:, None].astype(np.float64) * predict.soft_ce_grad(logits[0], labels[:, None], np.ones((B, 1)))
    assert rel(g, x.grad.numpy()) < 1e-12
    assert np.all(g[3] == 0)       # the zero-weight sample


def test_weighted_mean_of_the_soft_ce_rows_and_its_gradient():
    logits, _dp, _y, ids, w, _a, _t, _n = problem()
    s = weights()
    x = t64(logits[1], True)
    idt = torch.as_tensor(ids).long()
    aw = torch.where(idt > 0, t64(w), torch.zeros((), dtype=torch.float64))
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    rows = (aw * (lse - torch.gather(x, 1, (idt - 1).clamp(min=0)))).sum(1)
    obj = (t64(s) * rows).sum() / B
    obj.backward()
    assert rel(joint.weighted_mean(predict.soft_ce(logits[1], ids, w)[0], s), obj.item()) < 1e-6
    g = s[:, None].astype(np.float64) * predict.soft_ce_grad(logits[1], ids, w)
    assert rel(g, x.grad.numpy()) < 1e-12


@pytest.mark.parametrize("with_set", [False, True])
def test_weighted_mean_of_the_sigmoid_bce_rows_and_its_gradient(with_set):
    logits, _dp, labels, ids, w, _a, _t, _n = problem()
    s = weights()
    if not with_set:
        ids, w = labels[:, None], np.ones((B, 1), np.float32)
    x = t64(logits[2], True)
    tgt = t64(predict.bce_target(ids, w, K))
    live = t64((ids > 0).any(1).astype(np.float64)).unsqueeze(1)
    rows = (torch.nn.functional.binary_cross_entropy_with_logits(x, tgt, reduction="none") * live).sum(1)
    obj = (t64(s) * rows).sum() / B
    obj.backward()
    assert rel(joint.weighted_mean(predict.soft_bce(logits[2], ids, w, np.float64)[0], s), obj.item()) < 1e-12
    assert rel(joint.weighted_mean(predict.soft_bce(logits[2], ids, w)[0], s), obj.item()) < 1e-5
    g = s[:, None].astype(np.float64) * predict.soft_bce_grad(logits[2], ids, w, np.float64)
    assert rel(g, x.grad.numpy()) < 1e-12


def test_selection_bce_with_hop_times_sample_weights():
    _lg, dopred, _y, _ids, _w, _a, _t, _n = problem()
    s = weights()
    sel_w = np.array([0.7, 0.0, 1.3], np.float32)
    tg = (np.random.default_rng(4).uniform(size=(H, B)) > 0.5).astype(np.float32)
    x = t64(dopred, True)
    tt = t64(tg)
    rows = -(tt * torch.log(x + EPS) + (1 - tt) * torch.log(1 - x + EPS))             # [H, B]
    obj = (t64(sel_w)[:, None] * t64(s)[None, :] * rows).sum() / B
    obj.backward()
    W = joint.hop_sample_weights(sel_w, s)
    assert W.shape == (H, B) and W.dtype == np.float32
    assert np.array_equal(W, (sel_w[:, None] * s[None, :]).astype(np.float32))
    # the statement is nn.BCECriterion's -(t - x) / ((1 - x + eps)(x + eps)), autograd's the derivative of the loss with
    # its eps: they differ by eps / min(x, 1 - x) <= 1e-12 / 0.05 relative, so the fp64 bar is 1e-10, not 1e-12
    assert rel(joint.bce_grad(dopred.astype(np.float64), tg, joint.hop_sample_weights(sel_w, s, np.float64)),
               x.grad.numpy()) < 1e-10
    got = joint.bce_grad(dopred, tg, W)
    assert got.dtype == np.float32 and rel(got, x.grad.numpy()) < 1e-5
    assert np.all(got[:, 3] == 0) and np.all(got[1] == 0)
    # through the sigmoid: z with x = sigmoid(z)
    z = t64(np.log(dopred / (1 - dopred)), True)
    xs = torch.sigmoid(z)
    rows = -(tt * torch.log(xs + EPS) + (1 - tt) * torch.log(1 - xs + EPS))
    ((t64(sel_w)[:, None] * t64(s)[None, :] * rows).sum() / B).backward()
    sig = joint.select_signal(torch.sigmoid(z).detach().numpy(), tg, joint.hop_sample_weights(sel_w, s, np.float64))
    assert rel(sig, z.grad.numpy()) < 1e-10
    # per-row weighted loss
    for h in range(H):
        want = float((t64(s) * -(tt[h] * torch.log(t64(dopred[h]) + EPS)
                                 + (1 - tt[h]) * torch.log(1 - t64(dopred[h]) + EPS))).sum() / B)
        assert rel(joint.bce(dopred[h], tg[h], s), want) < 1e-5


@pytest.mark.parametrize("counts", [False, True])
def test_att_ce_and_its_gradient_with_weights(counts):
    _lg, _dp, _y, _ids, _w, att, t, nreg = problem()
    nreg = nreg if counts else None
    s = weights()
    att_w = np.array([0.5, 3.0, 1.5], np.float32)
    a = t64(att, True)
    tb = t64(t)
    if counts:
        tb = tb * (torch.arange(S)[None, :] < torch.as_tensor(nreg)[:, None])
    rows = (tb[None] * -torch.log(a + EPS)).sum(-1)                                    # [H, B]
    per_hop = (t64(s)[None, :] * rows).sum(-1) / B
    (t64(att_w) * per_hop).sum().backward()
    assert rel(joint.att_ce(att.astype(np.float64), t, nreg, sample_w=s), per_hop.detach().numpy()) < 1e-12
    assert rel(joint.att_ce(att, t, nreg, sample_w=s), per_hop.detach().numpy()) < 1e-5
    assert rel(joint.att_ce(att[0], t, nreg, sample_w=s), per_hop[0].item()) < 1e-5
    g64 = joint.att_ce_grad(att.astype(np.float64), t, joint.hop_sample_weights(att_w, s, np.float64), nreg)
    assert rel(g64, a.grad.numpy()) < 1e-12
    g = joint.att_ce_grad(att, t, joint.hop_sample_weights(att_w, s), nreg)
    assert g.dtype == np.float32 and rel(g, a.grad.numpy()) < 1e-5
    assert np.all(g[:, 3] == 0)
    st = joint.att_stats(att, t, nreg, sample_w=s)
    plain = joint.att_stats(att, t, nreg)
    assert rel(st["loss"], per_hop.detach().numpy()) < 1e-6
    assert np.array_equal(st["hits"], plain["hits"]) and st["n_sup"] == plain["n_sup"]
    assert np.array_equal(st["mass"], plain["mass"])


def test_feval_and_set_statistics_take_the_weight_per_row():
    logits, dopred, labels, ids, w, _a, _t, _n = problem()
    s = weights()
    plain = joint.feval_stats(logits, dopred, labels)
    got = joint.feval_stats(logits, dopred, labels, sample_w=s)
    for k in ("correct", "do_pred_correct", "did_correct", "fired", "selected"):
        assert np.array_equal(got[k], plain[k]), k
    uni, select, _hsel = joint.merged_rows(logits.astype(np.float64), dopred)
    rows = [logits[h].astype(np.float64) for h in range(H)] + [uni, select]
    y = torch.as_tensor(labels).long() - 1
    for r, row in enumerate(rows):
        want = float((t64(s) * torch.nn.functional.cross_entropy(t64(row), y, reduction="none")).sum() / B)
        assert rel(got["loss"][r], want) < 1e-5, r
    assert rel(got["loss"], plain["loss"]) > 1e-2          # the weights are at work
    for h in range(H):
        tg = (predict.first_max(logits[h]) == labels).astype(np.float32)
        assert got["loss_do_pred"][h] == joint.bce(dopred[h], tg, s)
    for loss in ("ce", "bce"):
        ps = predict.set_stats(logits, dopred, ids, w, loss=loss)
        gs = predict.set_stats(logits, dopred, ids, w, loss=loss, sample_w=s)
        for k in ("correct", "do_pred_correct", "did_correct", "fired", "selected", "ans", "score"):
            assert np.array_equal(gs[k], ps[k]), k
        row_loss = predict.soft_bce if loss == "bce" else predict.soft_ce
        for r, row in enumerate([logits[h] for h in range(H)] + [uni.astype(np.float32), select.astype(np.float32)]):
            assert rel(gs["loss"][r], joint.weighted_mean(row_loss(row, ids, w)[0], s)) < 1e-6


# ------------------------------------------------------------------------------------------ 2. normalize
def test_normalize_rescales_to_the_batch_size_in_float64():
    s = weights(seed=9, n=70)
    got = RAU._sample_weights(s, 70, normalize=True)
    assert got.dtype == np.float32 and got.shape == (70,)
    want = (s.astype(np.float64) * (70 / s.astype(np.float64).sum())).astype(np.float32)
    assert np.array_equal(got, want)
    assert abs(float(got.astype(np.float64).sum()) - 70) < 70 * 2.0 ** -23
    assert got[3] == 0
    same = RAU._sample_weights(s, 70)
    assert np.array_equal(same, s)                                     # never renormalised unless asked
    assert np.array_equal(RAU._sample_weights(np.full(5, 3.0), 5, True), np.ones(5, np.float32))
    assert RAU._sample_weights([1, 2, 3], 3).dtype == np.float32       # lists and integer arrays


# ------------------------------------------------------------------------------------------ 3. argument checks
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def _model(n):
    m = RAU.__new__(RAU)
    m._n, m._lib, m._h = n, _NoLibrary(), None
    return m


@pytest.mark.parametrize("bad,kw", [
    (np.ones(7, np.float32), {}),                         # one weight too few
    (np.ones((8, 1), np.float32), {}),                    # not a vector
    (np.array([1, 1, np.nan, 1, 1, 1, 1, 1], np.float32), {}),
    (np.array([1, 1, np.inf, 1, 1, 1, 1, 1], np.float32), {}),
    (np.array([1, 1, -0.5, 1, 1, 1, 1, 1], np.float32), {}),
    (np.zeros(8, np.float32), {"normalize": True}),       # nothing to normalise
])
def test_bad_weights_raise_before_the_library_is_touched(bad, kw):
    m = _model(8)
    with pytest.raises(ValueError):
        m.set_sample_weights(bad, **kw)
    with pytest.raises(ValueError):
        m.set_sample_weights(bad, slot=1, **kw)


def test_batch_uploads_check_the_weights_before_anything_moves():
    m = _model(8)
    lens = np.ones(8, np.int32)
    for call in (lambda: m.set_batch(None, None, lens, sample_w=np.ones(3)),
                 lambda: m.set_batch_async(0, lens=lens, sample_w=-np.ones(8)),
                 lambda: m.set_batch_async(1, sample_w=np.full(8, np.nan))):
        with pytest.raises(ValueError, match="sample weights"):
            call()
    with pytest.raises(AssertionError, match="the library was touched"):   # all-zero weights are legal without normalize
        m.set_sample_weights(np.zeros(8, np.float32))


# ------------------------------------------------------------------------------------------ 4. all ones
def test_all_ones_weights_reproduce_the_unweighted_statements_bit_for_bit():
    logits, dopred, labels, ids, w, att, t, nreg = problem()
    one = np.ones(B, np.float32)
    sel_w = np.array([0.7, 0.0, 1.3], np.float32)
    tg = (np.random.default_rng(4).uniform(size=(H, B)) > 0.5).astype(np.float32)
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    W = joint.hop_sample_weights(sel_w, one)
    assert np.array_equal(bits(joint.bce_grad(dopred, tg, W)), bits(joint.bce_grad(dopred, tg, sel_w)))
    assert np.array_equal(bits(joint.select_signal(dopred, tg, W)), bits(joint.select_signal(dopred, tg, sel_w)))
    for n in (None, nreg):
        assert np.array_equal(bits(joint.att_ce_grad(att, t, W, n)), bits(joint.att_ce_grad(att, t, sel_w, n)))
    for h in range(H):
        assert bits(joint.cross_entropy(logits[h], labels.astype(np.int64), one)) == \
            bits(joint.cross_entropy(logits[h], labels.astype(np.int64)))
        assert bits(joint.bce(dopred[h], tg[h], one)) == bits(joint.bce(dopred[h], tg[h]))
    a, b = joint.feval_stats(logits, dopred, labels, sample_w=one), joint.feval_stats(logits, dopred, labels)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for loss in ("ce", "bce"):
        a = predict.set_stats(logits, dopred, ids, w, loss=loss, sample_w=one)
        b = predict.set_stats(logits, dopred, ids, w, loss=loss)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    rows = predict.soft_ce(logits[0], ids, w)[0]
    assert np.array_equal(bits(joint.weighted_mean(rows, one)), bits(joint.weighted_mean(rows)))
    assert bits(joint.weighted_mean(rows)) == bits(predict.soft_ce(logits[0], ids, w)[1])
    for arr in (att, att.astype(np.float64), att[0]):           # att_ce keeps its one sum over samples and positions
        for n in (None, nreg):
            x, y = joint.att_ce(arr, t, n, sample_w=one), joint.att_ce(arr, t, n)
            assert x.dtype == y.dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes()
    for n in (None, nreg):
        x, y = joint.att_stats(att, t, n, sample_w=one), joint.att_stats(att, t, n)
        assert x["loss"].tobytes() == y["loss"].tobytes()
        assert np.array_equal(x["mass"], y["mass"]) and np.array_equal(x["hits"], y["hits"]) and x["n_sup"] == y["n_sup"]


# ------------------------------------------------------------------------------------------ 5. loader
from rau_vqa_amd import loader                                           # noqa: E402
from tests.test_loader import D as LD, H as LH, T as LT, W as LW, dataset   # noqa: E402,F401  (the fixture)


class _FakeRau:
    """The calls loader.feed and SlotFeeder make; records them in order."""

    def __init__(self, B):
        self.batch_size = B
        self.slots = [{"feats": np.zeros((B, LD, LW * LH), np.float32), "tokens": np.zeros((LT, B), np.int32),
                       "lens": np.zeros(B, np.int32), "labels": np.zeros(B, np.int32)} for _ in range(2)]
        self.log = []

    def batch_slot(self, s):
        return self.slots[s]

    def set_batch(self, *a, **kw):
        self.log.append(("set_batch", sorted(kw)))

    def set_batch_async(self, s, has_labels=True):
        self.log.append(("upload", s))

    def set_sample_weights(self, w, slot=-1):
        self.log.append(("weights", slot, np.array(w, copy=True)))

    def use_batch(self, s):
        self.log.append(("use", s))


def test_feed_attaches_the_weights_behind_the_batch(dataset):
    root, fdir, *_ = dataset
    B = 4
    d = loader.load_data(str(root), batch_size=B).train_data
    s = weights(n=B)
    rau = _FakeRau(B)
    loader.feed(rau, d.next_batch_feat(fdir, LD, LW, LH), sample_w=s)
    assert [e[0] for e in rau.log] == ["set_batch", "weights"]
    assert rau.log[1][1] == -1 and np.array_equal(rau.log[1][2], s)
    rau.log.clear()
    loader.feed(rau, d.next_batch_feat(fdir, LD, LW, LH))                 # None changes nothing
    assert [e[0] for e in rau.log] == ["set_batch"]
    # a dict batch: its own "sample_w" key travels to set_batch; the argument, when given, replaces it
    f, x, xl, a, qid = d.next_batch_feat(fdir, LD, LW, LH)
    batch = {"feats": f.reshape(B, LD, -1), "tokens": x, "lens": xl, "labels": a, "qids": qid, "sample_w": s}
    rau.log.clear()
    assert loader.feed(rau, batch) is qid
    assert rau.log == [("set_batch", ["feats", "labels", "lens", "sample_w", "tokens"])]
    rau.log.clear()
    loader.feed(rau, batch, sample_w=2 * s)
    assert rau.log[0] == ("set_batch", ["feats", "labels", "lens", "tokens"])
    assert rau.log[1][0] == "weights" and np.array_equal(rau.log[1][2], 2 * s)


def test_slot_feeder_sends_the_weights_of_every_batch_into_its_slot(dataset):
    """sample_w is a callable on the batch's question ids; the weights go up between the upload into the slot and
    use_batch, for every batch, in the slot of that batch."""
    root, fdir, *_ = dataset
    B = 4
    ref = loader.load_data(str(root), batch_size=B).train_data
    v = loader.load_data(str(root), batch_size=B)
    rau = _FakeRau(B)
    by_qid = lambda qids: (np.asarray(qids) % 7 / 3.0).astype(np.float32)
    feeder = loader.SlotFeeder(rau, v.train_data, fdir, LD, LW, LH, sample_w=by_qid)
    for it in range(7):                                                   # over the epoch wrap (23 examples / 4)
        qid = ref.next_batch_feat(fdir, LD, LW, LH)[4]
        up, w, use = rau.log[-3:]
        assert up == ("upload", it & 1) and use == ("use", it & 1)
        assert w[0] == "weights" and w[1] == (it & 1) and np.array_equal(w[2], by_qid(qid))
        assert np.array_equal(feeder.qids, qid)
        if it < 6:
            feeder.next()
    rau2 = _FakeRau(B)
    loader.SlotFeeder(rau2, loader.load_data(str(root), batch_size=B).train_data, fdir, LD, LW, LH)
    assert [e[0] for e in rau2.log] == ["upload", "use"]                  # without sample_w: nothing more
