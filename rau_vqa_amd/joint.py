"""Host restatement of feval's joint-loss bookkeeping (SS:476-556), line by line.

The reference's ``feval`` does more per iteration than the per-hop cross-entropy: it merges the hops
into a "uni" row (mean of the hop logits) and a "select" row (the logits of the first hop whose
do_pred fires; the last hop is NOT forced here, unlike predict_result), takes the CE and accuracy of
both, and scores every hop's do_pred with nn.BCECriterion against do_pred_gt = (argmax_h == y).
``RAU.step_stats`` computes the same numbers on the device (rau_step_stats); this module is the
plain float32 statement they are checked against.
"""
from __future__ import annotations

import numpy as np

from .predict import first_max

BCE_EPS = np.float32(1e-12)   # nn.BCECriterion's eps


def weighted_mean(rows, s=None):
    """(1/n) sum_b s_b rows[..., b]: what every built-in mean of the step path becomes under per-sample loss weights
    s [n] (rau_set_sample_weights; never renormalised).  Each product s_b * row is rounded once in the dtype of rows
    (float32 unless float64 is given), then the rows are summed and divided by n.  s None: the plain mean."""
    rows = _f32_unless_f64(rows)
    dt = rows.dtype
    if s is not None:
        rows = (np.asarray(s, dt) * rows).astype(dt)
    return (rows.sum(axis=-1, dtype=dt) / dt.type(rows.shape[-1])).astype(dt)


def cross_entropy(pred, y, sample_w=None):
    """nn.CrossEntropyCriterion (sizeAverage) of [B, K] float32 rows, y 1-based [B]; sample_w [B]: weighted_mean of
    the rows."""
    mx = pred.max(axis=1)
    lse = mx + np.log(np.exp(pred - mx[:, None]).sum(axis=1, dtype=np.float32))
    row = lse - pred[np.arange(pred.shape[0]), y - 1]
    if sample_w is not None:
        row = (np.asarray(sample_w, np.float32) * row).astype(np.float32)
    return np.float32(row.sum(dtype=np.float32) / np.float32(pred.shape[0]))


def bce(x, t, sample_w=None):
    """nn.BCECriterion (sizeAverage): -(t log(x + eps) + (1 - t) log(1 - x + eps)), mean over B; sample_w [B]:
    weighted_mean of the terms."""
    one = np.float32(1)
    term = -(t * np.log(x + BCE_EPS) + (one - t) * np.log(one - x + BCE_EPS))
    if sample_w is not None:
        term = (np.asarray(sample_w, np.float32) * term).astype(np.float32)
    return np.float32(term.sum(dtype=np.float32) / np.float32(x.shape[0]))


def _f32_unless_f64(a):
    a = np.asarray(a)
    return a if a.dtype == np.float64 else a.astype(np.float32)


def bce_grad(x, t, w):
    """nn.BCECriterion:backward (sizeAverage) scaled by w -- the reference's d_do_pred before its mul(0),
    SS:565-566, and the contract of rau_backward_select: w * (-(t - x) / ((1 - x + eps) * (x + eps))) / n, in
    this order, n = x.shape[-1].  x, t [..., n]; w a scalar, or [H] for [H, n] inputs, or [H, n]: hop weight times
    sample weight as ONE rounded product, select_w[h] * s_b (hop_sample_weights).  Float32 arithmetic (the
    device's), unless x is given as float64 (for references).  Torch tensors of one device are taken as they
    are: only arithmetic is used."""
    eps = float(BCE_EPS)
    if hasattr(x, "is_cuda"):
        return w * (-(t - x) / ((1 - x + eps) * (x + eps))) / float(x.shape[-1])
    x = _f32_unless_f64(x)
    t, w = np.asarray(t, x.dtype), np.asarray(w, x.dtype)
    if w.ndim == 1:
        w = w[:, None]
    one, eps = x.dtype.type(1), x.dtype.type(eps)
    return w * (-(t - x) / ((one - x + eps) * (x + eps))) / x.dtype.type(x.shape[-1])


def hop_sample_weights(w, s, dtype=np.float32):
    """[H, n] = w[h] * s[b], each product rounded once in dtype: the weight array bce_grad, select_signal and
    att_ce_grad take for a batch with per-sample loss weights s (the device's __fmul_rn(select_w[h], s_b))."""
    w, s = np.asarray(w, dtype), np.asarray(s, dtype)
    return (w[:, None] * s[None, :]).astype(dtype)


def select_signal(x, t, w):
    """bce_grad through the head's sigmoid: the gradient at Linear(M,1)'s output, s = ddp * x * (1 - x); w as in
    bce_grad (a scalar, [H] or [H, n])."""
    if not hasattr(x, "is_cuda"):
        x = _f32_unless_f64(x)
    return bce_grad(x, t, w) * x * (1 - x)


def ext_signal(ddp, x):
    """A gradient ddp at the do_pred output through the head's sigmoid: s_ext = (ddp * x) * (1 - x), in this order --
    the contract of rau_backward_ext's d_dopred, and select_signal's own last step (select_signal(x, t, w) is
    ext_signal(bce_grad(x, t, w), x) bit for bit).  Float32 arithmetic (the device's), unless x is given as
    float64 (for references)."""
    if not hasattr(x, "is_cuda"):
        x = _f32_unless_f64(x)
        ddp = np.asarray(ddp, x.dtype)
    return (ddp * x) * (1 - x)


def _att_valid(shape, nreg):
    """[..., n, S] bool: position s of sample b lies below its region count (None: every position)."""
    S = shape[-1]
    if nreg is None:
        return np.ones(shape[-2:], bool)
    n = np.clip(np.asarray(nreg, np.int64), 1, S)
    return np.arange(S)[None, :] < n[:, None]


def att_ce(a, t, nreg=None, sample_w=None):
    """The attention supervision's loss (rau_backward_att): ATT = (1/n) sum_b sum_{s < nreg[b]} t (-log(a + eps)).
    a [n, S] or [H, n, S] attention, t [n, S] targets >= 0, nreg [n] region counts or None -> a scalar, or [H].
    sample_w [n]: per-sample loss weights, ATT = (1/n) sum_b s_b sum_s term[b, s]: every term of sample b is
    multiplied by s_b (each product rounded once) and the sum is the unweighted one's, so weights all equal to 1 give
    the unweighted bits.  Float32 arithmetic unless a is given as float64."""
    a = _f32_unless_f64(a)
    t = np.where(_att_valid(a.shape, nreg), np.asarray(t, a.dtype), a.dtype.type(0))
    term = np.where(t > 0, t * -np.log(a + a.dtype.type(BCE_EPS)), a.dtype.type(0))
    if sample_w is not None:
        term = (np.asarray(sample_w, a.dtype)[:, None] * term).astype(a.dtype)
    return term.sum(axis=(-2, -1), dtype=a.dtype) / a.dtype.type(a.shape[-2])


def att_ce_grad(a, t, w, nreg=None):
    """d(w * att_ce)/da, the contract of rau_backward_att: -((w * t) / (a + eps)) / n in this order, n = a.shape[-2];
    exactly +0 where t == 0 or s >= nreg[b].  w a scalar, or [H] for [H, n, S] inputs, or [H, n]: hop weight times
    sample weight as one rounded product, att_w[h] * s_b (hop_sample_weights).  Float32 arithmetic (the device's),
    unless a is given as float64 (for references)."""
    a = _f32_unless_f64(a)
    t, w = np.asarray(t, a.dtype), np.asarray(w, a.dtype)
    if w.ndim == 1:
        w = w[:, None, None]
    elif w.ndim == 2:
        w = w[:, :, None]
    on = _att_valid(a.shape, nreg) & (t > 0)
    t = np.where(on, t, a.dtype.type(0))
    g = -((w * t) / (a + a.dtype.type(BCE_EPS))) / a.dtype.type(a.shape[-2])
    return np.where(on, g, a.dtype.type(0)).astype(a.dtype)


def att_stats(a, t, nreg=None, sample_w=None):
    """What RAU.att_stats reports, of a [H, n, S] against t [n, S] (nreg [n] or None), in float64: ``loss`` [H] =
    att_ce, ``mass`` [H] = mean over the supervised rows of the attention on the positions with t > 0, ``hits`` [H]
    = supervised rows whose first-max attention position has t > 0, ``n_sup`` = supervised rows (some t > 0 below
    the count).  Positions behind a count take no part.  sample_w [n]: ``loss`` takes s_b per row (att_ce's); mass,
    hits and n_sup stay unweighted."""
    a = np.asarray(a, np.float64)
    valid = _att_valid(a.shape, nreg)
    pos = (np.asarray(t) > 0) & valid                        # [n, S]
    sup = pos.any(axis=1)
    n_sup = int(sup.sum())
    loss = att_ce(a, np.asarray(t, np.float64), nreg, sample_w)
    mass = (a * pos).sum(axis=2)[:, sup].sum(axis=1) / max(n_sup, 1)
    arg = np.where(valid, a, -1.0).argmax(axis=2)            # first maximum below the count
    hit = np.take_along_axis(np.broadcast_to(pos, a.shape), arg[..., None], axis=2)[..., 0] & sup
    return {"loss": loss, "mass": mass, "hits": hit.sum(axis=1).astype(np.int32), "n_sup": n_sup}


def feval_stats(logits, dopred, labels, sample_w=None):
    """logits [H, B, K], dopred [H, B], labels [B] (1-based) -> dict with the keys of
    ``RAU.step_stats`` (loss [H+2], loss_do_pred [H], correct [H+2], do_pred_correct [H],
    did_correct, fired [H], selected [H]) plus ``uni_ans`` / ``select_ans`` [B].
    sample_w [B] (rau_set_sample_weights): every loss takes s_b per row; the counts stay unweighted."""
    logits = np.asarray(logits, np.float32)
    dopred = np.asarray(dopred, np.float32)
    y = np.asarray(labels, np.int64)
    H, B, K = logits.shape
    uni_pred = np.zeros((B, K), np.float32)                  # uni_pred:zero(), SS:474
    select_pred = np.zeros((B, K), np.float32)               # select_pred:zero(), SS:475
    did_pred = np.zeros(B, np.float32)                       # did_pred:zero(), SS:476
    did_correct = np.zeros(B, np.float32)                    # did_correct:zero(), SS:477
    tab_loss, tab_do_pred, tab_do_pred_gt = [], [], []
    correct, fired, selected = [], [], []
    for h in range(H):
        pred = logits[h]
        uni_pred += pred                                     # SS:482
        tab_do_pred.append(dopred[h])                        # SS:484
        ans = first_max(pred)                                # SS:488
        is_correct = (ans == y).astype(np.float32)           # SS:490
        correct.append(int(is_correct.sum()))                # SS:491
        tab_do_pred_gt.append(is_correct.copy())             # SS:497-498
        do_pred = (dopred[h] > 0.5).astype(np.float32)       # SS:501
        pred_cur_hop = np.clip(do_pred - did_pred, 0, 1)     # SS:505
        select_pred += pred * pred_cur_hop[:, None]          # SS:506-507
        fired.append(int(do_pred.sum()))
        selected.append(int(pred_cur_hop.sum()))
        did_correct = np.clip(did_correct + is_correct, 0, 1)   # SS:513
        did_pred = np.clip(did_pred + do_pred, 0, 1)         # SS:515
        tab_loss.append(cross_entropy(pred, y, sample_w))    # SS:518-519
    uni_pred = uni_pred / np.float32(H)                      # SS:522
    uni_ans = first_max(uni_pred)                            # SS:524
    correct.append(int((uni_ans == y).sum()))                # SS:526
    tab_loss.append(cross_entropy(uni_pred, y, sample_w))    # SS:529-530
    select_ans = first_max(select_pred)                      # SS:534
    correct.append(int((select_ans == y).sum()))             # SS:536
    tab_loss.append(cross_entropy(select_pred, y, sample_w))   # SS:539-540
    do_pred_correct, tab_loss_do_pred = [], []
    for h in range(H):
        do_pred = (tab_do_pred[h] > 0.5).astype(np.float32)  # SS:549
        do_pred_correct.append(int(((do_pred == tab_do_pred_gt[h]) * did_correct).sum()))   # SS:552
        tab_loss_do_pred.append(bce(tab_do_pred[h], tab_do_pred_gt[h], sample_w))            # SS:555
    return {"loss": np.array(tab_loss, np.float32), "loss_do_pred": np.array(tab_loss_do_pred, np.float32),
            "correct": np.array(correct, np.int32), "do_pred_correct": np.array(do_pred_correct, np.int32),
            "did_correct": int(did_correct.sum()), "fired": np.array(fired, np.int32),
            "selected": np.array(selected, np.int32), "uni_ans": uni_ans, "select_ans": select_ans}


def merged_rows(logits, dopred):
    """feval's two merged rows of logits [H, B, K] under do_pred [H, B], in the dtype of logits (float32 unless
    float64 is given): (uni [B, K], select [B, K], hsel [B]).  uni: sequential adds from 0, then a division by H
    (SS:482, 522); select: 0 + the logits of the first hop whose do_pred > 0.5 (SS:501-507, feval_stats' lines: the
    clamp(do - did) recurrence picks that hop, the last hop is NOT forced), all zeros on a row where none fired;
    hsel: that hop, -1 where none fired."""
    logits = _f32_unless_f64(logits)
    dt = logits.dtype
    H, B, K = logits.shape
    uni = np.zeros((B, K), dt)
    select = np.zeros((B, K), dt)
    did = np.zeros(B, bool)
    hsel = np.full(B, -1, np.int64)
    for h in range(H):
        uni += logits[h]                                     # SS:482
        do = np.asarray(dopred[h]) > 0.5                     # SS:501
        cur = do & ~did                                      # SS:505
        select += logits[h] * cur[:, None].astype(dt)        # SS:506-507
        hsel[cur] = h
        did |= do                                            # SS:515
    return uni / dt.type(H), select, hsel


def _ce_grad_rows(row, labels, answers):
    """d CE(row) / d row for rows [B, K] against labels [B] (1-based) or answers = (ids [B, G], w [B, G]): the
    criterion's gradient rule, softmax * (W_b / B) and then -= w_g / B at every non-empty entry in g order (a label
    is the set {y} with weight 1), in row's dtype."""
    dt = row.dtype
    B = row.shape[0]
    if answers is None:
        ids = np.asarray(labels, np.int64).reshape(B, 1)
        w = np.ones((B, 1), dt)
    else:
        ids = np.asarray(answers[0], np.int64)
        w = np.where(ids > 0, np.asarray(answers[1], dt), dt.type(0)).astype(dt)
    invB = dt.type(1) / dt.type(B)
    mx = row.max(axis=1, keepdims=True)
    ex = np.exp(row - mx)
    W = np.zeros(B, dt)
    for g in range(ids.shape[1]):
        W = W + w[:, g]
    out = ((ex / ex.sum(axis=1, keepdims=True, dtype=dt)) * (W * invB)[:, None]).astype(dt)
    ar = np.arange(B)
    for g in range(ids.shape[1]):
        live = ids[:, g] > 0
        out[ar[live], ids[live, g] - 1] -= (w[live, g] * invB).astype(dt)
    return out


def merged_ce_grad(logits, dopred, labels=None, answers=None, merge_w=(0.0, 0.0)):
    """The gradient of  merge_w[0] * CE(uni row, truth) + merge_w[1] * CE(select row, truth)  at the hop logits: the
    contract of rau_backward_merged / rau_merge_criterion_backward, as the [H, B, K] array they ADD to d_logits.

    logits [H, B, K], dopred [H, B]; truth is labels [B] (1-based) or answers = (ids [B, G], w [B, G]) (ids 1-based,
    0 = empty entry; the soft-target CE of predict.soft_ce).  The rows are merged_rows' (the feval rule: the numbers
    RAU.step_stats reports as loss[H] and loss[H+1]); CE is sizeAverage over the B rows.  With g(row) the criterion's
    gradient at a row (softmax - target, times 1/B; for a set softmax * W_b / B - sum_g onehot(y_g) w_g / B):
      uni     every hop h receives (merge_w[0] / H) * g(uni)[b, :]
      select  hop hsel(b) receives merge_w[1] * g(select)[b, :]; rows on which no hop fired receive exactly 0 in
              every hop (their select row is the constant zero row)
    and no gradient flows through the gate do_pred > 0.5.  Float32 arithmetic (the device's order: each product and
    sum rounded once, uni first), or float64 when logits is given as float64 (for references)."""
    logits = _f32_unless_f64(logits)
    dt = logits.dtype
    H, B, K = logits.shape
    if (labels is None) == (answers is None):
        raise ValueError("merged_ce_grad: give labels or answers")
    w_uni, w_sel = dt.type(merge_w[0]), dt.type(merge_w[1])
    uni, select, hsel = merged_rows(logits, dopred)
    out = np.zeros((H, B, K), dt)
    if w_uni != 0:
        out += ((w_uni / dt.type(H)) * _ce_grad_rows(uni, labels, answers))[None]
    if w_sel != 0:
        g_s = w_sel * _ce_grad_rows(select, labels, answers)
        fired = np.nonzero(hsel >= 0)[0]
        out[hsel[fired], fired] += g_s[fired]
    return out


def image_hop_sum(G, keep, p, S, Sp, image_of, n_images, order=None):
    """The per-image feature-map gradient dT [n_images, D, Sp] float32 (rau_set_feat_grad, RAU_FEAT_GRAD_IMAGES) from
    the per-hop, per-sample products G [HA, n, D, Sp] (pad columns of any content), the keep bits keep [HA, n, D, S]
    over the LOGICAL tensor, indexed by SAMPLE (None: no mask, scale 1) and the drop probability p.  The device's
    arithmetic: the hops in `order` (default ascending); per hop the accumulator starts at +0 (the first hop) or at
    the stored value, an image's samples are taken in ascending b, each term keep ? G * s_x : 0 rounded once to
    float32 and then added.  An image no sample names stays exactly zero; pad columns are zero."""
    G = np.asarray(G, np.float32)
    HA, n, D, _ = G.shape
    image_of = np.asarray(image_of, np.int64)
    if image_of.shape != (n,) or (n and (image_of.min() < 0 or image_of.max() >= n_images)):
        raise ValueError(f"image_of must be [{n}] with entries in [0, {n_images})")
    s_x = np.float32(1.0) if keep is None else np.float32(1.0 / (1.0 - p))
    out = np.zeros((n_images, D, Sp), np.float32)
    for h in (range(HA) if order is None else order):
        for b in range(n):
            term = G[h, b, :, :S] * s_x
            if keep is not None:
                term = np.where(np.asarray(keep[h][b]).reshape(D, S) != 0, term, np.float32(0))
            out[image_of[b], :, :S] += term
    return out
