"""The fp64 whole-step reference for multiple-choice candidates (rau_set_candidates), built on the unchanged oracle.

It is tests/ext_ref.step called on the batch WITHOUT labels and hop weights, with the restricted criterion handed over
as its callable F -- the method of tests/test_gpu_sample_weights.py:

    F = sum_h hop_w[h] * (1/n) sum_b s_b row_b(scores_h)  (+ a term of the caller's own)

row_b is stated here on the hop scores with torch alone, independently of rau_vqa_amd/predict.py.  L_b is the SET of
non-zero candidate ids of sample b (so a duplicate counts once), the kept truth the set entries -- or the label as the
one-entry set {(y, 1)} -- whose id lies in L_b:

    softmax   row_b = sum_{kept g} w_g (logsumexp_{k in L_b} x_k - x[y_g])
    sigmoid   row_b = sum_{k in L_b} binary_cross_entropy_with_logits(x_k, t_k),  t_k = min(1, sum of kept w_g on k)

A row without a kept entry contributes nothing.  select_w / t_gt, att_w / att_t and nreg pass through to ext_ref.step's
own terms.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import ext_ref


def live_mask(cand, K):
    """[B, K] bool: answer k is a candidate of sample b (ids 1-based, 0 = empty entry)"""
    cand = np.asarray(cand)
    mask = np.zeros((cand.shape[0], K), bool)
    for b, row in enumerate(cand):
        for c in row:
            if c > 0:
                mask[b, c - 1] = True
    return mask


def rows_fn(sh, batch, cand, answers=None, loss="ce"):
    """scores [B, K] fp64 (with their graph) -> the restricted criterion's rows [B]"""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    K = sh.K
    mask = live_mask(cand, K)
    if answers is not None:
        ids, w = np.asarray(answers[0], np.int64), np.asarray(answers[1], np.float64)
    else:
        ids, w = np.asarray(batch["labels"], np.int64)[:, None], np.ones((sh.B, 1))
    kept = (ids > 0) & mask[np.arange(sh.B)[:, None], np.maximum(ids, 1) - 1]
    w = np.where(kept, w, 0.0)
    labelled = kept.any(axis=1)
    safe = mask | ~labelled[:, None]            # rows that contribute nothing keep a finite logsumexp
    mk, sf, wk = torch.as_tensor(mask), torch.as_tensor(safe), t(w)
    col = torch.as_tensor(np.maximum(ids, 1) - 1)
    lab = t(labelled.astype(np.float64))
    if loss == "bce":
        tgt = np.zeros((sh.B, K))
        for b in range(sh.B):
            for g in range(ids.shape[1]):
                if kept[b, g]:
                    tgt[b, ids[b, g] - 1] += w[b, g]
        tgt = t(np.minimum(tgt, 1.0))
        return lambda sc: (torch.nn.functional.binary_cross_entropy_with_logits(sc, tgt, reduction="none")
                           * mk).sum(1) * lab
    return lambda sc: (wk * (torch.logsumexp(sc.masked_fill(~sf, -np.inf), dim=1, keepdim=True)
                             - torch.gather(sc, 1, col))).sum(1) * lab


def objective(sh, batch, cand, hop_w, s=None, answers=None, loss="ce", extra=None, keep=None):
    """F for ext_ref.step; keep["rows"]: the (weighted) criterion rows per hop; extra: one more callable, added."""
    rows = rows_fn(sh, batch, cand, answers, loss)
    sv = torch.ones(sh.B, dtype=torch.float64) if s is None else torch.as_tensor(np.asarray(s, np.float64))

    def F(scores, dps, atts):
        total = 0.0
        for h in range(sh.H):
            r = sv * rows(scores[h])
            if keep is not None:
                keep.setdefault("rows", []).append(r.detach().numpy())
            total = total + float(hop_w[h]) * r.sum() / sh.B
        if extra is not None:
            total = total + extra(scores, dps, atts)
        return total
    return F


def step(sh, params, batch, masks, cand, hop_w, s=None, answers=None, loss="ce", bf16=False, extra=None, **terms):
    """One step of the restricted objective; ext_ref.step's result plus rows [H, n], the criterion rows."""
    keep = {}
    F = objective(sh, batch, cand, hop_w, s, answers, loss, extra, keep)
    ref = ext_ref.step(sh, params, dict(batch, labels=None), masks, None, F=F, bf16=bf16, **terms)
    ref["rows"] = np.stack(keep["rows"][:sh.H])
    return ref
