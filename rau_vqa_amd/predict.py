"""Inference path: the reference's ``predict_result`` (SS:633-705) and the answer
selection of its eval loop (SS:877-897) on top of ``rau_forward`` in evaluate mode.

The heavy part (encoder + H hops; in evaluate mode dropout is the identity, so
i_embed and the attention pre-activation are hop-invariant and computed once) runs
in librau.so.  What is left is bookkeeping on [H,B,K] / [H,B,S] host arrays:
``do_pred > 0.5`` thresholding, "select" (first hop whose do_pred fires, last hop
forced, SS:683-688) and "uni" (mean over hops, SS:699-700) merging, multiple-choice
masking and first-max argmax.  The reference's quirks are reproduced, not fixed:
MC masking multiplies the RAW logits by a 0/1 mask (SS:894), so masked-out answers
become 0 and can beat negative valid logits.
"""
from __future__ import annotations

import numpy as np


def merge_hops(logits, dopred, att, select_att_state=None):
    """tab_pred / tab_att of SS:690-704: H per-hop entries, then uni, then select.

    select_att_state: the reference zeroes test_select_pred, test_uni_* and test_did_pred at the
    top of predict_result (SS:671-674) but NOT test_select_att, so its "select" attention map
    keeps accumulating across batches (it only feeds the attention PNGs).  Pass the array a
    previous call returned as tab_att[-1] to reproduce that; None starts from zeros (what the
    first batch sees)."""
    H, B, K = logits.shape
    did = np.zeros(B, np.float32)                       # test_did_pred:zero(), SS:674
    select_pred = np.zeros((B, K), np.float32)
    select_att = (np.zeros((B, att.shape[2]), np.float32) if select_att_state is None
                  else np.array(select_att_state, np.float32))   # never zeroed, SS:671-674
    for h in range(H):
        do = (dopred[h] > 0.5).astype(np.float32)       # SS:683
        if h == H - 1:
            do[:] = 1.0                                 # always predict in the final step, SS:685
        cur = np.clip(do - did, 0.0, 1.0)               # SS:686
        select_pred += logits[h] * cur[:, None]         # SS:687
        select_att += att[h] * cur[:, None]             # SS:688
        did = np.clip(did + do, 0.0, 1.0)               # SS:697
    uni_pred = logits.sum(0, dtype=np.float32) / np.float32(H)   # SS:680, 699
    uni_att = att.sum(0, dtype=np.float32) / np.float32(H)       # SS:681, 700
    tab_pred = [logits[h] for h in range(H)] + [uni_pred, select_pred]
    tab_att = [att[h] for h in range(H)] + [uni_att, select_att]
    return tab_pred, tab_att


def first_max(x):
    """torch.max(x, 2) index: FIRST maximal entry, 1-based (SS:896, 900)."""
    return np.argmax(x, axis=1).astype(np.int32) + 1


def answers(tab_pred, mc_ans=None):
    """Open-ended and multiple-choice answer ids (1-based) per entry of tab_pred.

    mc_ans: int array [B, nMultChoice] of candidate answer ids, 0 = empty slot
    (loader.lua:96, 1377).  Returns (oe [H+2, B], mc [H+2, B] or None).
    """
    oe = np.stack([first_max(p) for p in tab_pred])
    if mc_ans is None:
        return oe, None
    B, K = tab_pred[0].shape
    mask = np.zeros((B, K), np.float32)                 # test_mc_mask, SS:886-893
    for b in range(B):
        for a in mc_ans[b]:
            if a != 0:
                mask[b, a - 1] = 1.0
    mc = np.stack([first_max(p * mask) for p in tab_pred])   # cmul on raw logits, SS:894
    return oe, mc


def rank_key(x):
    """uint64 key whose DESCENDING order is the total order of rau_dev_topk / rau_topk on the f32
    entries of x [..., K]: the high word is the monotone unsigned image of the float with -0
    canonicalised to +0 and NaN below -inf, the low word is 0xffffffff - index, so equal values
    order by the lower index and no two keys of a row are equal."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    hi = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    hi = np.where(nan, np.uint32(0), hi).astype(np.uint64)
    lo = np.uint64(0xffffffff) - np.arange(u.shape[-1], dtype=np.uint64)
    return (hi << np.uint64(32)) | lo


def top_answers(tab_pred, k):
    """The k best answers of every row of tab_pred ([R, B, K] or a list of R [B, K] arrays, as
    merge_hops returns): (ids int32 1-based, score f32, conf f32), each [R, B, k], best first -- the
    numpy statement of rau_topk's contract.  Larger value first; equal values (+0 == -0) by the lower
    id, which extends first_max (SS:896, 900) to every rank; NaN after -inf, by the lower id.  score
    is the entry itself, bit for bit; conf is the row's softmax probability, exp(score - max) /
    sum exp(v - max) in float64, rounded to f32 at the end (defined for finite rows)."""
    x = np.ascontiguousarray(np.stack([np.asarray(p, np.float32) for p in tab_pred]))
    K = x.shape[-1]
    if not 1 <= k <= K:
        raise ValueError(f"k={k} out of [1,{K}]")
    # a stable sort of the inverted key; keys are distinct, so stability only guards the statement
    order = np.argsort(~rank_key(x), axis=-1, kind="stable")[..., :k]
    score = np.take_along_axis(x, order, axis=-1)
    with np.errstate(invalid="ignore", over="ignore"):
        x64 = x.astype(np.float64)
        mx = np.take_along_axis(x64, order[..., :1], axis=-1)
        e = np.exp(x64 - mx)
        conf = np.exp(score.astype(np.float64) - mx) / e.sum(-1, keepdims=True)
    return (order + 1).astype(np.int32), score, conf.astype(np.float32)


def soft_ce(pred, ids, w):
    """Criterion of rau_set_answers on rows pred [B, K] float32 against the answer set ids [B, G] (1-based, 0 =
    empty entry), w [B, G]: (rows [B] float32, their mean) with rows[b] = sum_g w[b,g] (lse_b - pred[b, y_g]),
    every operation in float32, accumulated from 0 in g order.  G = 1, w = 1 is joint.cross_entropy."""
    pred = np.asarray(pred, np.float32)
    ids = np.asarray(ids, np.int64)
    w = np.asarray(w, np.float32)
    B = pred.shape[0]
    mx = pred.max(axis=1)
    lse = mx + np.log(np.exp(pred - mx[:, None]).sum(axis=1, dtype=np.float32))
    rows = np.zeros(B, np.float32)
    ar = np.arange(B)
    for g in range(ids.shape[1]):
        live = ids[:, g] > 0
        term = w[:, g] * (lse - pred[ar, np.maximum(ids[:, g], 1) - 1])
        rows = np.where(live, rows + term, rows).astype(np.float32)
    return rows, np.float32(rows.sum(dtype=np.float32) / np.float32(B))


def soft_ce_grad(pred, ids, w):
    """d mean(soft_ce rows) / d pred as the device forms it: softmax * (W_b / B) - sum_g onehot(y_g) w_g / B,
    W_b = the row's summed non-empty weights (float64: a reference, not a bit statement)."""
    pred = np.asarray(pred, np.float64)
    ids = np.asarray(ids, np.int64)
    w = np.where(ids > 0, np.asarray(w, np.float64), 0.0)
    B = pred.shape[0]
    e = np.exp(pred - pred.max(axis=1, keepdims=True))
    g = e / e.sum(axis=1, keepdims=True) * w.sum(axis=1, keepdims=True) / B
    for b in range(B):
        for j in range(ids.shape[1]):
            if ids[b, j] > 0:
                g[b, ids[b, j] - 1] -= w[b, j] / B
    return g


def bce_target(ids, w, K):
    """Target of the per-answer sigmoid criterion (rau_set_answer_loss, RAU_LOSS_BCE) for the answer set ids [B, G]
    (1-based, 0 = empty entry; clamped into [0, K] as the device clamps them), w [B, G]: t [B, K] float32 with
    t[b, k] = min(1, sum_g w[b, g] [ids[b, g] - 1 == k]) over the non-empty entries, added from 0 in g order in
    float32, then clamped.  Bit for bit the device's target."""
    ids = np.clip(np.asarray(ids, np.int64), 0, K)
    w = np.asarray(w, np.float32)
    B = ids.shape[0]
    t = np.zeros((B, K), np.float32)
    ar = np.arange(B)
    for g in range(ids.shape[1]):
        live = ids[:, g] > 0
        col = np.maximum(ids[:, g], 1) - 1
        t[ar[live], col[live]] = t[ar[live], col[live]] + w[live, g]     # one entry per row: no aliasing
    return np.minimum(t, np.float32(1))


def bce_target_labels(labels, K):
    """bce_target of the one-entry sets {(y, 1)}: t[b, k] = [k == y_b - 1], labels 1-based, clamped into [1, K]."""
    y = np.clip(np.asarray(labels, np.int64), 1, K)
    return bce_target(y[:, None], np.ones((y.shape[0], 1), np.float32), K)


def _block_sum(terms):
    """Sum over the last axis in the order of the device's criterion heads: 256 partials, partial i adding the
    entries i, i + 256, .. in ascending order from 0, then an xor butterfly over each group of 64 partials (offsets
    32 .. 1) and (w0 + w1) + (w2 + w3).  In the dtype of terms."""
    K = terms.shape[-1]
    pad = (-K) % 256
    x = np.concatenate([terms, np.zeros(terms.shape[:-1] + (pad,), terms.dtype)], axis=-1)
    x = x.reshape(terms.shape[:-1] + (-1, 256))
    part = np.zeros(terms.shape[:-1] + (256,), terms.dtype)
    for i in range(x.shape[-2]):
        part = part + x[..., i, :]
    v = part.reshape(terms.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    wv = v[..., 0]
    return (wv[..., 0] + wv[..., 1]) + (wv[..., 2] + wv[..., 3])


def soft_bce(pred, ids, w, dtype=np.float32):
    """The per-answer sigmoid criterion of RAU_LOSS_BCE on rows pred [B, K] against the answer set ids / w [B, G]:
    (rows [B], their mean) with rows[b] = sum_k max(x,0) - x t + log1p(exp(-|x|)), t = bce_target -- summed over K,
    not divided by K.  A row whose set has no non-empty entry is unlabelled: 0.  Labels y [B]: ids = y[:, None],
    w = 1.  dtype float32 (the default) computes every step in float32 and sums in the device's order; the
    exponential and the logarithm are numpy's, so this is a reference to a few ulp, not a bit statement."""
    x = np.asarray(pred, dtype)
    K = x.shape[1]
    t = bce_target(ids, w, K).astype(dtype)
    e = np.exp(-np.abs(x))
    term = ((np.maximum(x, 0) - x * t) + np.log1p(e)).astype(dtype)
    rows = _block_sum(term)
    rows = np.where((np.asarray(ids) > 0).any(axis=1), rows, 0).astype(dtype)
    return rows, dtype(rows.sum(dtype=dtype) / dtype(x.shape[0]))


def soft_bce_grad(pred, ids, w, dtype=np.float32):
    """d mean(soft_bce rows) / d pred as the device forms it: (sigmoid(x) - t) / B with the sigmoid from
    e = exp(-|x|) as x >= 0 ? 1 / (1 + e) : e / (1 + e) -- finite for every finite x; +0 on unlabelled rows."""
    x = np.asarray(pred, dtype)
    B, K = x.shape
    t = bce_target(ids, w, K).astype(dtype)
    e = np.exp(-np.abs(x))
    d = dtype(1) + e
    sg = np.where(x >= 0, dtype(1) / d, e / d).astype(dtype)
    g = ((sg - t) * (dtype(1) / dtype(B))).astype(dtype)
    return np.where((np.asarray(ids) > 0).any(axis=1)[:, None], g, dtype(0)).astype(dtype)


def answer_score(ans, ids, score):
    """Metric score of the answers ans [..., B] (1-based) against the set: sum_g score[b,g] * [ids[b,g] == ans],
    float32, added from 0 in g order; empty entries (id 0) never match.  Bit for bit what rau_step_scores /
    rau_predict_scores return for the device's own answers."""
    ans = np.asarray(ans, np.int64)
    ids = np.asarray(ids, np.int64)
    score = np.asarray(score, np.float32)
    out = np.zeros(ans.shape, np.float32)
    for g in range(ids.shape[1]):
        hit = (ids[:, g] > 0) & (ans == ids[:, g])
        out = np.where(hit, out + score[:, g], out).astype(np.float32)
    return out


def set_correct(ans, ids, score):
    """The "correct" rule of a batch with an answer set: the answer is among the row's non-empty ids with
    score > 0 (never on a row without entries).  Boolean, shape of ans."""
    ans = np.asarray(ans, np.int64)
    ids = np.asarray(ids, np.int64)
    score = np.asarray(score, np.float32)
    ok = np.zeros(ans.shape, bool)
    for g in range(ids.shape[1]):
        ok |= (ids[:, g] > 0) & (score[:, g] > 0) & (ans == ids[:, g])
    return ok


def feval_rows(logits, dopred):
    """feval's merged rows of hop logits [H, B, K] float32 (SS:482-540; the last hop is NOT forced): (uni, select,
    first) with uni = (0 + l_0 + .. + l_{H-1}) / H, select = 0 + l_first on the rows where a hop fired (the zero row
    elsewhere) and first [B] the first hop whose do_pred > 0.5, -1 when none fires.  Bit for bit the device's rows."""
    logits = np.asarray(logits, np.float32)
    H, B, K = logits.shape
    fire = np.asarray(dopred, np.float32) > 0.5
    first = np.where(fire.any(0), fire.argmax(0), -1)              # feval: the last hop is not forced
    uni = np.zeros((B, K), np.float32)
    for h in range(H):
        uni += logits[h]
    uni = uni / np.float32(H)
    select = np.zeros((B, K), np.float32)
    for b in range(B):
        if first[b] >= 0:
            select[b] = np.float32(0) + logits[first[b], b]
    return uni, select, first


def set_stats(logits, dopred, ids, w, score=None, loss="ce", sample_w=None):
    """joint.feval_stats for a batch with an answer set (rau_step_stats with a set): the same keys, with
    set_correct in place of (argmax == y) and soft_ce in place of the cross-entropy, plus ``score`` [H+2, B]:
    answer_score of every row's answer (what rau_step_scores returns).  loss="bce": the statistics of a step under
    RAU_LOSS_BCE -- ``loss`` is soft_bce of every row; everything else does not depend on the criterion.
    sample_w [B] (rau_set_sample_weights): every loss is the mean of s_b * row (each product rounded once in
    float32); the counts and the scores stay unweighted."""
    if loss not in ("ce", "bce"):
        raise ValueError(f"loss={loss!r}: 'ce' or 'bce'")
    row_loss = soft_bce if loss == "bce" else soft_ce
    logits = np.asarray(logits, np.float32)
    dopred = np.asarray(dopred, np.float32)
    score = np.asarray(w if score is None else score, np.float32)
    H, B, K = logits.shape
    eps, one = np.float32(1e-12), np.float32(1)
    fire = dopred > 0.5
    uni, select, first = feval_rows(logits, dopred)
    rows = [logits[h] for h in range(H)] + [uni, select]
    ans = np.stack([first_max(r) for r in rows])
    ok = set_correct(ans, ids, score)
    did = ok[:H].any(0)
    sw = None if sample_w is None else np.asarray(sample_w, np.float32)

    def mean(r):   # (1/B) sum_b s_b r_b
        r = r if sw is None else (sw * r).astype(np.float32)
        return np.float32(r.sum(dtype=np.float32) / np.float32(B))
    loss = np.array([row_loss(r, ids, w)[1] if sw is None else mean(row_loss(r, ids, w)[0]) for r in rows],
                    np.float32)
    ldp, dpc = [], []
    for h in range(H):
        t = ok[h].astype(np.float32)
        x = dopred[h]
        term = -(t * np.log(x + eps) + (one - t) * np.log(one - x + eps))
        ldp.append(mean(term))
        dpc.append(int(((fire[h] == ok[h]) & did).sum()))
    return {"loss": loss, "loss_do_pred": np.array(ldp, np.float32), "correct": ok.sum(1).astype(np.int32),
            "do_pred_correct": np.array(dpc, np.int32), "did_correct": int(did.sum()),
            "fired": fire.sum(1).astype(np.int32),
            "selected": np.array([(first == h).sum() for h in range(H)], np.int32),
            "ans": ans, "score": answer_score(ans, ids, score)}


def predict_result(rau, feats, tokens, lens, mc_ans=None, select_att_state=None, image_of=None):
    """SS:633-705 + SS:877-900 for one batch: returns dict(tab_pred, tab_att, oe, mc).
    select_att_state: see merge_hops (carry tab_att[-1] from batch to batch to reproduce the
    reference's never-zeroed test_select_att).  image_of: feats is an image table (RAU.set_batch)."""
    rau.evaluate()
    rau.set_batch(feats, tokens, lens, None, image_of=image_of)
    rau.forward()
    tab_pred, tab_att = merge_hops(rau.logits(), rau.dopred(), rau.attention(), select_att_state)
    oe, mc = answers(tab_pred, mc_ans)
    return {"tab_pred": tab_pred, "tab_att": tab_att, "oe": oe, "mc": mc}


def predict_result_device(rau, feats, tokens, lens, mc_ans=None, select_att_state=None, tabs=True,
                          image_of=None, topk=None):
    """predict_result with the merges, the MC masking and the answers done on the device
    (rau_predict): same keys, same values bit for bit.  The select attention row comes back without
    the reference's carried test_select_att; select_att_state is added here, as merge_hops does.
    tabs=False skips downloading the per-hop logits and maps: tab_pred / tab_att are then None and
    only the answers (and nothing of [H, B, K]) cross PCIe.  image_of: as in predict_result.
    Like predict_result it takes batches below the context's capacity (the test split's 83 rows on a
    context trained at 100): set_batch switches the context to lens.shape[0] rows first.
    topk=k adds top_ids, top_score, top_conf [H+2, B, k] (rau_topk: the k best open-ended answers of
    every row with their logits and softmax confidences; top_answers states them in numpy)."""
    rau.evaluate()
    rau.set_batch(feats, tokens, lens, None, image_of=image_of)
    rau.forward()
    oe, mc = rau.predict(mc_ans)
    top = {}
    if topk is not None:
        top["top_ids"], top["top_score"], top["top_conf"] = rau.topk(topk)
    if not tabs:
        return {"tab_pred": None, "tab_att": None, "oe": oe, "mc": mc, **top}
    pred, att = rau.merged()
    if select_att_state is not None:
        att[1] = np.array(select_att_state, np.float32) + att[1]   # never zeroed, SS:671-674
    logits, hop_att = rau.logits(), rau.attention()
    H = logits.shape[0]
    tab_pred = [logits[h] for h in range(H)] + [pred[0], pred[1]]
    tab_att = [hop_att[h] for h in range(H)] + [att[0], att[1]]
    return {"tab_pred": tab_pred, "tab_att": tab_att, "oe": oe, "mc": mc, **top}


# ---- multiple-choice candidates (rau_set_candidates): the numpy statement of the restricted criterion, the ranked
# candidates and the MC statistics.  cand [B, C] int, 1-based answer ids, 0 = empty entry.

def cand_live(cand):
    """[B, C] bool: the live entries of a candidate list -- non-empty and equal to no EARLIER entry of the row (a
    duplicate id counts once)."""
    cand = np.asarray(cand, np.int64)
    live = cand > 0
    for c in range(1, cand.shape[1]):
        live[:, c] &= ~(cand[:, :c] == cand[:, c:c + 1]).any(axis=1)
    return live


def cand_kept(cand, ids):
    """[B, G] bool: the kept truth -- set entries (labels y: ids = y[:, None]) that are non-empty and whose id is a
    live candidate of the row.  The others count as empty entries; a row without a kept entry is unlabelled."""
    cand = np.asarray(cand, np.int64)
    ids = np.asarray(ids, np.int64)
    live = cand_live(cand)
    inl = ((ids[:, :, None] == cand[:, None, :]) & live[:, None, :]).any(axis=2)
    return (ids > 0) & inl


def _cand_args(logits, cand, ids, w, sample_w, dtype):
    x = np.asarray(logits, dtype)
    B, K = x.shape
    cand = np.clip(np.asarray(cand, np.int64), 0, K)
    ids = np.clip(np.asarray(ids, np.int64), 0, K)
    if ids.ndim == 1:
        ids = ids[:, None]
    w = np.ones(ids.shape, dtype) if w is None else np.asarray(w, dtype)
    if cand.ndim != 2 or cand.shape[0] != B or ids.shape[0] != B or w.shape != ids.shape:
        raise ValueError("cand must be [B, C], ids and w [B, G] for logits [B, K]")
    sw = np.ones(B, dtype) if sample_w is None else np.asarray(sample_w, dtype)
    return x, cand, ids, w, sw, cand_live(cand), cand_kept(cand, ids)


def _cand_lse(x, cols, dtype):
    """m, den, lse of x over the columns `cols` (entry order): den added from +0 in that order, each step rounded once"""
    m = x[cols].max()
    den = dtype(0)
    for c in cols:
        den = dtype(den + np.exp(dtype(x[c] - m)))
    return m, den, dtype(m + np.log(den))


def cand_ce(logits, cand, ids, w=None, sample_w=None, dtype=np.float32):
    """The softmax criterion restricted to candidates (rau_set_candidates) on rows logits [B, K] against the answer
    set ids / w [B, G] (labels y [B]: ids = y, w = None): (rows [B], their mean) with, over the live candidates L of
    a row in entry order, m = max x_c, den = sum expf(x_c - m), lse = m + log(den) and rows[b] = s_b * sum_g w_g
    (lse - x[y_g]) over the KEPT entries (cand_kept) from 0 in g order.  A row without a kept entry: 0.  Every step
    in `dtype` and in the device's order; exp and log are numpy's, so float32 is a reference to a few ulp."""
    x, cand, ids, w, sw, live, kept = _cand_args(logits, cand, ids, w, sample_w, dtype)
    B = x.shape[0]
    rows = np.zeros(B, dtype)
    for b in range(B):
        if not kept[b].any():
            continue
        _, _, lse = _cand_lse(x[b], cand[b][live[b]] - 1, dtype)
        acc = dtype(0)
        for g in np.nonzero(kept[b])[0]:
            acc = dtype(acc + dtype(w[b, g] * dtype(lse - x[b, ids[b, g] - 1])))
        rows[b] = dtype(sw[b] * acc)
    return rows, dtype(rows.sum(dtype=dtype) / dtype(B))


def cand_ce_grad(logits, cand, ids, w=None, sample_w=None, dtype=np.float32):
    """d mean(cand_ce rows) / d logits [B, K] as the device forms it: for k in L (expf(x_k - m) / den) (W invB), then for
    the kept g in order: if (y_g == k) -= w_g invB, the first match inside a fused multiply-add; +0 outside L and on
    rows without a kept entry.  invB = s_b * (1 / B), W = the kept weights added in order."""
    x, cand, ids, w, sw, live, kept = _cand_args(logits, cand, ids, w, sample_w, dtype)
    B = x.shape[0]
    g_out = np.zeros(x.shape, dtype)
    for b in range(B):
        if not kept[b].any():
            continue
        cols = cand[b][live[b]] - 1
        m, den, _ = _cand_lse(x[b], cols, dtype)
        invB = dtype(sw[b] * dtype(dtype(1) / dtype(B)))
        W = dtype(0)
        for g in np.nonzero(kept[b])[0]:
            W = dtype(W + w[b, g])
        scale = dtype(W * invB)
        for k in cols:
            e = dtype(np.exp(dtype(x[b, k] - m)) / den)
            p, hit = dtype(e * scale), False
            for g in np.nonzero(kept[b])[0]:
                if ids[b, g] - 1 == k:
                    wb = dtype(w[b, g] * invB)
                    p = dtype(p - wb) if hit else dtype(np.float64(e) * np.float64(scale) - np.float64(wb))
                    hit = True
            g_out[b, k] = p
    return g_out


def _cand_bce_rows(x, cand, ids, w, live, kept, b, dtype):
    """(cols, t, e) of row b: its live candidates' columns, their targets over the kept entries, expf(-|x|)"""
    cols = cand[b][live[b]] - 1
    t = np.zeros(len(cols), dtype)
    for i, k in enumerate(cols):
        for g in np.nonzero(kept[b])[0]:
            if ids[b, g] - 1 == k:
                t[i] = dtype(t[i] + w[b, g])
    return cols, np.minimum(t, dtype(1)), np.exp(-np.abs(x[b, cols]))


def cand_bce(logits, cand, ids, w=None, sample_w=None, dtype=np.float32):
    """The per-answer sigmoid criterion restricted to candidates: (rows [B], their mean) with rows[b] = s_b *
    sum_{c in L} (max(x_c,0) - x_c t_c) + log1p(exp(-|x_c|)), added from 0 in entry order, t_c = min(1, the kept
    matching weights added in order).  A row without a kept entry is unlabelled: 0."""
    x, cand, ids, w, sw, live, kept = _cand_args(logits, cand, ids, w, sample_w, dtype)
    B = x.shape[0]
    rows = np.zeros(B, dtype)
    for b in range(B):
        if not kept[b].any():
            continue
        cols, t, e = _cand_bce_rows(x, cand, ids, w, live, kept, b, dtype)
        xc = x[b, cols]
        term = ((np.maximum(xc, 0) - (xc * t).astype(dtype)).astype(dtype) + np.log1p(e)).astype(dtype)
        acc = dtype(0)
        for v in term:
            acc = dtype(acc + v)
        rows[b] = dtype(sw[b] * acc)
    return rows, dtype(rows.sum(dtype=dtype) / dtype(B))


def cand_bce_grad(logits, cand, ids, w=None, sample_w=None, dtype=np.float32):
    """d mean(cand_bce rows) / d logits [B, K]: (sigmoid(x_c) - t_c) invB at the live candidates' columns, the sigmoid
    from e = exp(-|x|) as x >= 0 ? 1 / (1 + e) : e / (1 + e); +0 elsewhere and on unlabelled rows."""
    x, cand, ids, w, sw, live, kept = _cand_args(logits, cand, ids, w, sample_w, dtype)
    B = x.shape[0]
    g_out = np.zeros(x.shape, dtype)
    for b in range(B):
        if not kept[b].any():
            continue
        cols, t, e = _cand_bce_rows(x, cand, ids, w, live, kept, b, dtype)
        xc = x[b, cols]
        d = (dtype(1) + e).astype(dtype)
        sg = np.where(xc >= 0, dtype(1) / d, e / d).astype(dtype)
        invB = dtype(sw[b] * dtype(dtype(1) / dtype(B)))
        g_out[b, cols] = ((sg - t).astype(dtype) * invB).astype(dtype)
    return g_out


def top_candidates(tab_pred, cand, k):
    """The k best CANDIDATES of every row of tab_pred ([R, B, K] or a list of R [B, K] arrays, the merged rows
    top_answers reads): (ids int32 1-based, score f32, conf f32), each [R, B, k] -- the numpy statement of
    rau_topk_cand.  A row's live candidates (cand_live) are ranked among themselves in top_answers' total order
    (rank_key: larger value first, ties by the lower answer id, NaN last); score is the row's entry, bit for bit;
    conf = exp(v - m) / sum_{c in L} exp(x_c - m) in float64, rounded to f32 at the end.  Ranks at and behind the
    number of live candidates: id 0, score -inf, conf 0.  Rank 0 is the first maximum of the candidates' logits; the
    reference's multiply rule (answers(tab_pred, mc_ans)) agrees with it whenever that logit is positive."""
    x = np.ascontiguousarray(np.stack([np.asarray(p, np.float32) for p in tab_pred]))
    R, B, K = x.shape
    cand = np.asarray(cand, np.int64)
    if cand.ndim != 2 or cand.shape[0] != B:
        raise ValueError(f"cand must be [{B}, C]")
    C = cand.shape[1]
    if not 1 <= k <= C:
        raise ValueError(f"k={k} out of [1,{C}]")
    if cand.min() < 0 or cand.max() > K:
        raise ValueError(f"candidate id outside [0,{K}]")
    live = cand_live(cand)
    key = rank_key(x)
    ids = np.zeros((R, B, k), np.int32)
    score = np.full((R, B, k), -np.inf, np.float32)
    conf = np.zeros((R, B, k), np.float32)
    for b in range(B):
        cols = cand[b][live[b]] - 1
        if len(cols) == 0:
            continue
        for r in range(R):
            order = cols[np.argsort(~key[r, b, cols], kind="stable")]
            v = x[r, b, order]
            n = min(k, len(order))
            ids[r, b, :n] = order[:n] + 1
            score[r, b, :n] = v[:n]
            with np.errstate(invalid="ignore", over="ignore"):
                v64 = x[r, b, cols].astype(np.float64)
                m = v64.max()
                conf[r, b, :n] = (np.exp(v[:n].astype(np.float64) - m) / np.exp(v64 - m).sum()).astype(np.float32)
    return ids, score, conf


def _wave_total(x):
    """Sum over the last axis in the order of the device's batch totals (rau_step_scores, rau_cand_stats): 64 partials,
    partial l adding the entries l, l + 64, .. in ascending order from 0, then an xor butterfly (offsets 32 .. 1)."""
    x = np.asarray(x, np.float32)
    pad = (-x.shape[-1]) % 64
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), np.float32)], axis=-1).reshape(x.shape[:-1] + (-1, 64))
    v = np.zeros(x.shape[:-2] + (64,), np.float32)
    for i in range(x.shape[-2]):
        v = v + x[..., i, :]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def cand_stats(logits, dopred, cand, ids, w=None, score=None, loss="ce", sample_w=None):
    """The MC statistics of a step on a batch with candidates (rau_cand_stats), feval rule: for every row of
    {hops, uni, select} (feval_rows) ``loss`` [H+2] = the mean of cand_ce (loss="bce": cand_bce) with the sample
    weights, ``correct`` [H+2] = the labelled rows whose rank-0 candidate (top_candidates) carries a positive score in
    the set, ``score`` [H+2] = that candidate's summed metric score (added in the device's fixed order), ``n_lab`` = the rows with a kept truth entry,
    ``ans`` [H+2, B] the rank-0 candidates.  Labels y [B]: ids = y, w = score = None (weight and score 1)."""
    if loss not in ("ce", "bce"):
        raise ValueError(f"loss={loss!r}: 'ce' or 'bce'")
    logits = np.asarray(logits, np.float32)
    H, B, K = logits.shape
    ids = np.asarray(ids, np.int64)
    if ids.ndim == 1:
        ids = ids[:, None]
    w = np.ones(ids.shape, np.float32) if w is None else np.asarray(w, np.float32)
    score = np.asarray(w if score is None else score, np.float32)
    uni, select, _ = feval_rows(logits, dopred)
    rows = [logits[h] for h in range(H)] + [uni, select]
    row_loss = cand_bce if loss == "bce" else cand_ce
    lab = cand_kept(cand, ids).any(axis=1)
    ans = top_candidates(rows, cand, 1)[0][:, :, 0]
    sc = np.where(lab[None, :], answer_score(ans, ids, score), np.float32(0)).astype(np.float32)
    return {"loss": np.array([row_loss(r, cand, ids, w, sample_w)[1] for r in rows], np.float32),
            "correct": (sc > 0).sum(1).astype(np.int32), "score": _wave_total(sc),
            "n_lab": int(lab.sum()), "ans": ans}
