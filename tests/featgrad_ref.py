"""Reference for the feature-map gradient (rau_set_feat_grad), built on the unchanged oracle/ref_torch.py.

att_ref._forward restated with the feature maps as ONE fp64 leaf that requires grad (every per-sample run of a batch
with region counts slices the same leaf), on ref_torch's own multimodal, deep_lstm and _drop; otherwise the objective
is ext_ref.step's

    sum_h hop_w[h] * CE_h  +  F(scores, dps, atts)

(CE: cross_entropy, or under loss="bce" bce_ref's criterion; F a callable on the outputs WITH their graphs, None is no
such term; a batch without labels has no criterion).  step() returns ext_ref.step's outputs, g_<group> and g_feats
[B, D, S], the gradient at the maps.  pre(feats) -> feats', a differentiable torch function, stands for a trainable
stage in front of the library: the leaf is then ITS input and g_feats the gradient there; g_pre holds the gradients
of the tensors in pre_params.

masked_hop_sum() is the numpy statement of what the device forms from the per-hop products.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle.ref_torch import _drop, _split, deep_lstm, mult_specs, multimodal, rnn_specs
from tests import att_ref, bce_ref

GROUPS = ("embed", "rnn", "mult")


def _forward(sh, flat, feats, batch, masks, rows, n_b, bf16, dtype):
    """att_ref._forward with the maps read from the tensor `feats` [B, D, S] (with its graph)."""
    t = lambda a: torch.as_tensor(a).to(dtype)
    Emb = flat["embed"].view(sh.V, sh.E)
    Pr = _split(flat["rnn"], rnn_specs(sh))
    Pm = dict(_split(flat["mult"], mult_specs(sh)))
    if n_b is not None:
        live = torch.arange(sh.S) < int(n_b)
        Pm["att_mem.b"] = torch.where(live, Pm["att_mem.b"], torch.full((), att_ref.MASKED, dtype=dtype))
    B = rows.stop - rows.start
    shb = dataclasses.replace(sh, B=B)
    feats4d = feats[rows].reshape(B, sh.D, sh.S, 1)
    tokens = torch.as_tensor(np.ascontiguousarray(batch["tokens"][:, rows])).long()
    lens = torch.as_tensor(batch["lens"][rows]).long()
    mk = lambda k: None if masks is None else torch.as_tensor(np.ascontiguousarray(masks[k][:, rows]))
    m_we, m_rnn, m_q, m_x, m_mf = mk("we"), mk("rnn"), mk("q"), mk("x"), mk("mf")
    Q = 4 * sh.Rq
    state = torch.zeros(B, Q, dtype=dtype)
    q = torch.zeros(B, Q, dtype=dtype)
    for tt in range(1, int(lens.max()) + 1):
        we = torch.tanh(_drop(Emb[tokens[tt - 1] - 1], None if m_we is None else m_we[tt - 1], sh.p_we))
        state = deep_lstm(shb, Pr, we, state, None if m_rnn is None else m_rnn[tt - 1])
        q = torch.where((lens == tt).unsqueeze(1), state, q)
    c = torch.zeros(B, sh.R, dtype=dtype)
    h = torch.zeros(B, sh.R, dtype=dtype)
    hops = []
    for hop in range(sh.H):
        score, dp, a, c, h = multimodal(
            shb, Pm, q, feats4d, c, h,
            None if m_q is None else m_q[hop],
            None if m_x is None else m_x[hop].reshape(B, sh.D, sh.S, 1),
            None if m_mf is None else m_mf[hop], bf16=bf16)
        hops.append((score, dp, a))
    return hops


def step(sh, params, batch, masks, hop_w, bf16=False, F=None, nreg=None, loss="ce", pre=None, pre_params=()):
    dtype = torch.float64
    t = lambda a: torch.as_tensor(a).to(dtype)
    flat = {k: t(params[k]).clone().requires_grad_(True) for k in GROUPS}
    leaf = t(batch["feats"]).clone().requires_grad_(True)
    feats = leaf if pre is None else pre(leaf)
    B = sh.B
    parts = [(slice(0, B), None)] if nreg is None else [(slice(b, b + 1), int(nreg[b])) for b in range(B)]
    per_hop = [[] for _ in range(sh.H)]
    for rows, n_b in parts:
        for hop, vals in enumerate(_forward(sh, flat, feats, batch, masks, rows, n_b, bf16, dtype)):
            per_hop[hop].append(vals)
    cat = lambda hop, i: (per_hop[hop][0][i] if len(parts) == 1 else torch.cat([v[i] for v in per_hop[hop]], 0))
    scores = [cat(hop, 0) for hop in range(sh.H)]
    dps = [cat(hop, 1) for hop in range(sh.H)]
    atts = [cat(hop, 2) for hop in range(sh.H)]
    ce = None
    if batch.get("labels") is not None and loss == "bce":
        tgt, lab = bce_ref.target(sh, batch, None)
        tgt, live = t(tgt), t(lab.astype(np.float64)).unsqueeze(1)
        ce = lambda score: (torch.nn.functional.binary_cross_entropy_with_logits(score, tgt, reduction="none")
                            * live).sum() / B
    elif batch.get("labels") is not None:
        y = torch.as_tensor(batch["labels"]).long() - 1
        ce = lambda score: torch.nn.functional.cross_entropy(score, y)
    total = 0.0
    for hop in range(sh.H):
        if ce is not None and hop_w is not None:
            total = total + float(hop_w[hop]) * ce(scores[hop])
        else:
            assert hop_w is None or float(hop_w[hop]) == 0.0, "a hop weight on a batch without labels"
    ext = F(scores, dps, atts) if F is not None else None
    if ext is not None:
        total = total + ext
    res = {"logits": np.stack([s.detach().numpy() for s in scores]),
           "dopred": np.stack([d.detach().numpy() for d in dps]),
           "att": np.stack([a.detach().numpy() for a in atts]),
           "ext": 0.0 if ext is None else float(ext.detach())}
    total.backward()
    for k in GROUPS:
        g = flat[k].grad
        res["g_" + k] = (torch.zeros_like(flat[k]) if g is None else g).detach().numpy()
    res["g_feats"] = (torch.zeros_like(leaf) if leaf.grad is None else leaf.grad).detach().numpy()
    res["g_pre"] = [p.grad.detach().numpy() for p in pre_params]
    return res


def masked_hop_sum(G, keep, p, S, Sp, order=None):
    """dX [n, D, Sp] float32 from the per-hop products G [HA, n, D, Sp] (pad columns of any content), the keep bits
    keep [HA, n, D, S] over the LOGICAL tensor (None: no mask, scale 1) and the drop probability p: each term
    keep * (G * s_x) rounded once, added in `order` (default ascending) from the first term, pad columns zero --
    k_xgrad_accum's arithmetic."""
    G = np.asarray(G, np.float32)
    HA, n, D, _ = G.shape
    s_x = np.float32(1.0) if keep is None else np.float32(1.0 / (1.0 - p))
    out = np.zeros((n, D, Sp), np.float32)
    for i, h in enumerate(range(HA) if order is None else order):
        term = G[h, :, :, :S] * s_x
        if keep is not None:
            term = np.where(np.asarray(keep[h]).reshape(n, D, S) != 0, term, np.float32(0))
        out[:, :, :S] = term if i == 0 else out[:, :, :S] + term
    return out
