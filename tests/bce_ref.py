"""Reference for the per-answer sigmoid criterion (rau_set_answer_loss, RAU_LOSS_BCE), built on the unchanged
oracle/ref_torch.py.

ref_torch._step restated (as tests/merge_ref.py and tests/att_ref.py restate it) on ref_torch's own multimodal,
deep_lstm, _drop, _split and specs, in fp64 autograd with explicit masks (None: evaluate mode), with the answer
criterion of every hop

    binary_cross_entropy_with_logits(score, t, reduction="sum") / B

summed over K and not divided by K; t [B, K] comes from predict.bce_target (an answer set) or
predict.bce_target_labels, and the rows of samples without a non-empty entry are zeroed: such a sample is unlabelled,
its loss is 0 and it hands back no gradient.  select_w with t_gt [H, B] (do_pred_gt from the device's argmax) adds
the BCE term of rau_backward_select, as merge_ref.step does.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.ref_torch import _drop, _split, deep_lstm, mult_specs, multimodal, rnn_specs
from rau_vqa_amd import predict

GROUPS = ("embed", "rnn", "mult")
EPS = 1e-12


def target(sh, batch, answers=None):
    """(t [B, K] float64, labelled [B] bool): the criterion's target for the batch's labels or its answer set."""
    if answers is None:
        return predict.bce_target_labels(batch["labels"], sh.K).astype(np.float64), np.ones(sh.B, bool)
    ids, w = answers[0], answers[1]
    return predict.bce_target(ids, w, sh.K).astype(np.float64), (np.asarray(ids) > 0).any(axis=1)


def step(sh, params, batch, masks, hop_w, select_w=None, t_gt=None, answers=None, bf16=False, backward=True):
    """One step under the sigmoid criterion.  Returns logits, dopred, argmax, losses [H] and, with backward,
    g_<group> of  sum_h hop_w[h] * BCE_h (+ select_w[h] * BCE_eps(do_pred_h, t_gt[h]))."""
    dtype = torch.float64
    t = lambda a: torch.as_tensor(a).to(dtype)
    flat = {k: t(params[k]).clone().requires_grad_(backward) for k in GROUPS}
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
    tgt, labelled = target(sh, batch, answers)
    tgt, live = t(tgt), t(labelled.astype(np.float64)).unsqueeze(1)

    def bce(score):
        rows = torch.nn.functional.binary_cross_entropy_with_logits(score, tgt, reduction="none") * live
        return rows.sum() / B
    scores, dps, losses, total = [], [], [], 0.0
    for hop in range(sh.H):
        score, dp, _a, c, h = multimodal(
            sh, Pm, q, feats4d, c, h,
            None if m_q is None else m_q[hop],
            None if m_x is None else m_x[hop].reshape(sh.B, sh.D, sh.S, 1),
            None if m_mf is None else m_mf[hop], bf16=bf16)
        scores.append(score)
        dps.append(dp)
        loss = bce(score)
        losses.append(float(loss.detach()))
        total = total + float(hop_w[hop]) * loss
        if select_w is not None and t_gt is not None:
            tg = t(t_gt[hop])
            sel = -(tg * torch.log(dp + EPS) + (1 - tg) * torch.log(1 - dp + EPS)).mean()
            total = total + float(select_w[hop]) * sel
    res = {"logits": np.stack([s.detach().numpy() for s in scores]),
           "dopred": np.stack([d.detach().numpy() for d in dps]),
           "losses": np.array(losses)}
    res["argmax"] = np.argmax(res["logits"], axis=-1) + 1
    if backward:
        total.backward()
        for k in GROUPS:
            g = flat[k].grad
            res["g_" + k] = (torch.zeros_like(flat[k]) if g is None else g).numpy()
    return res
