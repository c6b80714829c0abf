"""Reference for custom objectives (rau_backward_ext), built on the unchanged oracle/ref_torch.py.

ref_torch._step restated (as tests/merge_ref.py, tests/att_ref.py and tests/bce_ref.py restate it) on ref_torch's own
multimodal, deep_lstm, _drop, _split and specs, in fp64 autograd with explicit masks (None: evaluate mode).  The
objective is merge_ref.step's, with att_ref.step's attention term, plus a term of the caller's own:

    sum_h ( hop_w[h] * CE_h + select_w[h] * BCE_eps(do_pred_h, t_h) + att_w[h] * ATT_h )
      + w_uni * CE(uni row) + w_sel * CE(select row)  +  F(scores, dps, atts)

F is a Python callable on three lists of H fp64 tensors WITH their graphs: scores [B, K], dps [B], atts [B, S].  It
returns a scalar tensor; None is no such term.  The built-in terms are stated exactly as merge_ref.step and
att_ref.step state them (CE is cross_entropy, with an answer set predict.soft_ce's statement, under loss="bce"
bce_ref.step's criterion), so that F = None reproduces them.  A batch without labels (batch["labels"] None) has no
criterion: every built-in term but the attention's must then be absent.

With region counts the forward runs once per sample on a B = 1 shape with attbymemory.linear's bias at -1e30 behind
the count (att_ref._forward, the method of tests/regions_ref.py); the per-sample outputs are concatenated WITH their
graphs into [B, ..] tensors, and every term above is taken on those.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import att_ref, bce_ref, merge_ref

GROUPS = ("embed", "rnn", "mult")
EPS = 1e-12


def step(sh, params, batch, masks, hop_w, merge_w=None, select_w=None, t_gt=None, answers=None, bf16=False,
         backward=True, F=None, att_w=None, att_t=None, nreg=None, loss="ce"):
    """One step of the objective above.  Returns logits [H,B,K], dopred [H,B], att [H,B,S], argmax, gate (first_fire of
    its own do_pred), ext (F's value, 0.0 without one) and, with backward, g_<group>."""
    dtype = torch.float64
    t = lambda a: torch.as_tensor(a).to(dtype)
    flat = {k: t(params[k]).clone().requires_grad_(backward) for k in GROUPS}
    B = sh.B
    parts = [(slice(0, B), None)] if nreg is None else [(slice(b, b + 1), int(nreg[b])) for b in range(B)]
    per_hop = [[] for _ in range(sh.H)]
    for rows, n_b in parts:
        hops, _q = att_ref._forward(sh, flat, batch, masks, rows, n_b, bf16, dtype)
        for hop, vals in enumerate(hops):
            per_hop[hop].append(vals[:3])
    cat = lambda hop, i: (per_hop[hop][0][i] if len(parts) == 1 else torch.cat([v[i] for v in per_hop[hop]], 0))
    scores = [cat(hop, 0) for hop in range(sh.H)]
    dps = [cat(hop, 1) for hop in range(sh.H)]
    atts = [cat(hop, 2) for hop in range(sh.H)]

    labelled = batch.get("labels") is not None
    ce = None
    if labelled and loss == "bce":
        tgt, lab = bce_ref.target(sh, batch, answers)
        tgt, live = t(tgt), t(lab.astype(np.float64)).unsqueeze(1)
        ce = lambda score: (torch.nn.functional.binary_cross_entropy_with_logits(score, tgt, reduction="none")
                            * live).sum() / B
    elif labelled and answers is not None:
        ids = torch.as_tensor(answers[0]).long()
        aw = torch.where(ids > 0, t(answers[1]), torch.zeros((), dtype=dtype))
        ce = lambda score: merge_ref.soft_ce(score, ids, aw, B)
    elif labelled:
        y = torch.as_tensor(batch["labels"]).long() - 1
        ce = lambda score: torch.nn.functional.cross_entropy(score, y)

    total = 0.0
    for hop in range(sh.H):
        if ce is not None:
            total = total + float(hop_w[hop]) * ce(scores[hop])
        else:
            assert hop_w is None or float(hop_w[hop]) == 0.0, "a hop weight on a batch without labels"
        if select_w is not None and t_gt is not None:
            tg = t(t_gt[hop])
            dp = dps[hop]
            bce = -(tg * torch.log(dp + EPS) + (1 - tg) * torch.log(1 - dp + EPS)).mean()
            total = total + float(select_w[hop]) * bce
        if att_w is not None and att_t is not None:
            tb = t(att_t)
            if nreg is not None:
                tb = tb * (torch.arange(sh.S)[None, :] < torch.as_tensor(np.asarray(nreg))[:, None])
            total = total + float(att_w[hop]) * ((tb * -torch.log(atts[hop] + EPS)).sum() / B)
    res = {"logits": np.stack([s.detach().numpy() for s in scores]),
           "dopred": np.stack([d.detach().numpy() for d in dps]),
           "att": np.stack([a.detach().numpy() for a in atts])}
    res["argmax"] = np.argmax(res["logits"], axis=-1) + 1
    res["gate"] = merge_ref.first_fire(res["dopred"])
    if merge_w is not None:
        assert ce is not None and loss == "ce", "the merged rows' terms are cross-entropies against labels"
        gate = t(res["gate"])                                              # detached: a constant
        uni = torch.stack(scores).mean(dim=0)
        select = sum(scores[hop] * gate[hop].unsqueeze(1) for hop in range(sh.H))
        total = total + float(merge_w[0]) * ce(uni) + float(merge_w[1]) * ce(select)
    ext = F(scores, dps, atts) if F is not None else None
    res["ext"] = 0.0 if ext is None else float(ext.detach())
    if ext is not None:
        total = total + ext
    if backward:
        if torch.is_tensor(total) and total.requires_grad:
            total.backward()
        for k in GROUPS:
            g = flat[k].grad
            res["g_" + k] = (torch.zeros_like(flat[k]) if g is None else g).detach().numpy()
    return res


def linear_F(G_l=None, G_d=None, G_a=None):
    """F = sum_h <G_l[h], logits_h> + <G_d[h], dopred_h> + <G_a[h], att_h> for fixed arrays G ([H,B,K], [H,B], [H,B,S];
    None: no such sum): its gradients at the outputs are the G themselves."""
    def F(scores, dps, atts):
        tot = 0.0
        for G, outs in ((G_l, scores), (G_d, dps), (G_a, atts)):
            if G is not None:
                for h, o in enumerate(outs):
                    tot = tot + (torch.as_tensor(np.asarray(G[h], np.float64)) * o).sum()
        return tot
    return F
