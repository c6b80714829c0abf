"""Reference for the merged answers as training terms (rau_backward_merged), built on the unchanged oracle/ref_torch.py.

ref_torch._step restated (as tests/test_gpu_select.py::oracle_step and tests/att_ref.py restate it) on ref_torch's
own multimodal, deep_lstm, _drop, _split and specs, in fp64 autograd with explicit masks, and with

    w_uni * CE(mean_h score_h)  +  w_sel * CE(sum_h score_h * gate_h)

added to  sum_h hop_w[h] * CE_h + select_w[h] * BCE_eps(do_pred_h, t_h).  gate_h [B] is the DETACHED first-fire
indicator of do_pred > 0.5 (feval's clamp(do - did) recurrence, SS:501-515; the last hop is not forced): no gradient
flows through it, and a row on which no hop fired has the constant zero select row.  CE is
torch.nn.functional.cross_entropy, or with an answer set predict.soft_ce's statement in torch: sum_g w (lse - score[y_g])
over the non-empty entries, mean over the batch.

first_fire() and fire_histogram() state the condition the GPU tests assert: the device's gates equal the oracle's, and
the batch holds a row that first fires at hop 0, one at a later hop and one that never fires.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.ref_torch import _drop, _split, deep_lstm, mult_specs, multimodal, rnn_specs

GROUPS = ("embed", "rnn", "mult")
EPS = 1e-12


def first_fire(dopred):
    """gate [H, B] 0/1: hop h is the first hop of row b with do_pred > 0.5 (at most one 1 per row)."""
    do = np.asarray(dopred) > 0.5
    did = np.zeros(do.shape[1], bool)
    gate = np.zeros(do.shape, np.float64)
    for h in range(do.shape[0]):
        gate[h] = do[h] & ~did
        did |= do[h]
    return gate


def fire_histogram(gate):
    """{'never': rows on which no hop fired, h: rows that first fire at hop h}"""
    out = {"never": int((gate.sum(0) == 0).sum())}
    for h in range(gate.shape[0]):
        out[h] = int(gate[h].sum())
    return out


def soft_ce(score, ids, aw, B):
    """predict.soft_ce's mean in torch: sum_b sum_g w (lse_b - score[b, y_g]) / B over the non-empty entries"""
    lse = torch.logsumexp(score, dim=1, keepdim=True)
    return (aw * (lse - torch.gather(score, 1, (ids - 1).clamp(min=0)))).sum() / B


def step(sh, params, batch, masks, hop_w, merge_w=None, select_w=None, t_gt=None, answers=None, bf16=False,
         backward=True):
    """One step with the merged terms.  merge_w None: none of them; select_w with t_gt [H, B] (do_pred_gt from the
    device's argmax): the BCE term of rau_backward_select; answers = (ids, w).  Returns logits, dopred, argmax, gate
    (first_fire of its own do_pred), merged_losses (CE of the uni and the select row) and, with backward, g_<group>."""
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
    y = torch.as_tensor(batch["labels"]).long() - 1
    if answers is not None:
        ids = torch.as_tensor(answers[0]).long()
        aw = torch.where(ids > 0, t(answers[1]), torch.zeros((), dtype=dtype))
        ce = lambda score: soft_ce(score, ids, aw, B)
    else:
        ce = lambda score: torch.nn.functional.cross_entropy(score, y)
    scores, dps, total = [], [], 0.0
    for hop in range(sh.H):
        score, dp, _a, c, h = multimodal(
            sh, Pm, q, feats4d, c, h,
            None if m_q is None else m_q[hop],
            None if m_x is None else m_x[hop].reshape(sh.B, sh.D, sh.S, 1),
            None if m_mf is None else m_mf[hop], bf16=bf16)
        scores.append(score)
        dps.append(dp)
        total = total + float(hop_w[hop]) * ce(score)
        if select_w is not None and t_gt is not None:
            tg = t(t_gt[hop])
            bce = -(tg * torch.log(dp + EPS) + (1 - tg) * torch.log(1 - dp + EPS)).mean()
            total = total + float(select_w[hop]) * bce
    res = {"logits": np.stack([s.detach().numpy() for s in scores]),
           "dopred": np.stack([d.detach().numpy() for d in dps])}
    res["argmax"] = np.argmax(res["logits"], axis=-1) + 1
    res["gate"] = first_fire(res["dopred"])
    gate = t(res["gate"])                                                  # detached: a constant
    uni = torch.stack(scores).mean(dim=0)
    select = sum(scores[hop] * gate[hop].unsqueeze(1) for hop in range(sh.H))
    ce_u, ce_s = ce(uni), ce(select)
    res["merged_losses"] = np.array([float(ce_u.detach()), float(ce_s.detach())])
    if backward:
        if merge_w is not None:
            total = total + float(merge_w[0]) * ce_u + float(merge_w[1]) * ce_s
        total.backward()
        for k in GROUPS:
            g = flat[k].grad
            res["g_" + k] = (torch.zeros_like(flat[k]) if g is None else g).numpy()
    return res
