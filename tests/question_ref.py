"""Reference for the question state from the caller (rau_set_question_dev), built on the unchanged oracle/ref_torch.py.

featgrad_ref._forward with the encoder loop removed: q [B, Q] comes from ONE fp64 leaf that requires grad (every
per-sample run of a batch with region counts slices the same leaf), the hops are ref_torch's own multimodal.  The
objective is featgrad_ref.step's

    sum_h hop_w[h] * CE_h  +  F(scores, dps, atts)

(CE: cross_entropy, or under loss="bce" bce_ref's criterion; F a callable on the outputs WITH their graphs; region
counts through att_ref.MASKED).  step() returns the outputs, g_mult, g_q [B, Q] (the gradient at the leaf) and, when
asked (want_feats), g_feats.  pre_q(z) -> q, a differentiable torch function, stands for the caller's question
encoder: the leaf is then ITS input z, g_q the gradient there, and g_pre holds the gradients of the tensors in
pre_params.

encoder_q() is ref_torch's own question encoder (embed, deep_lstm, length select) as such a function: with it in
front, step() is ref_torch's full step -- which is how tests/test_question_host.py shows that the cut is where the
oracle has it.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle.ref_torch import _drop, _split, deep_lstm, mult_specs, multimodal, rnn_specs
from tests import att_ref, bce_ref


def encoder_q(sh, embed_flat, rnn_flat, batch, masks, dtype=torch.float64):
    """q [B, Q] of ref_torch's encoder from the flat EMBED / RNN parameter tensors (with their graphs): the loop of
    ref_torch._step / featgrad_ref._forward, nothing else."""
    Emb = embed_flat.view(sh.V, sh.E)
    Pr = _split(rnn_flat, rnn_specs(sh))
    tokens = torch.as_tensor(np.ascontiguousarray(batch["tokens"])).long()
    lens = torch.as_tensor(batch["lens"]).long()
    m_we = None if masks is None else torch.as_tensor(masks["we"])
    m_rnn = None if masks is None else torch.as_tensor(masks["rnn"])
    Q = 4 * sh.Rq
    state = torch.zeros(sh.B, Q, dtype=dtype)
    q = torch.zeros(sh.B, Q, dtype=dtype)
    for tt in range(1, int(lens.max()) + 1):
        we = torch.tanh(_drop(Emb[tokens[tt - 1] - 1], None if m_we is None else m_we[tt - 1], sh.p_we))
        state = deep_lstm(sh, Pr, we, state, None if m_rnn is None else m_rnn[tt - 1])
        q = torch.where((lens == tt).unsqueeze(1), state, q)
    return q


def _forward(sh, Pm, q, feats, masks, rows, n_b, bf16, dtype):
    """featgrad_ref._forward without the encoder: q [B, Q] and feats [B, D, S] are tensors with their graphs."""
    Pm = dict(Pm)
    if n_b is not None:
        live = torch.arange(sh.S) < int(n_b)
        Pm["att_mem.b"] = torch.where(live, Pm["att_mem.b"], torch.full((), att_ref.MASKED, dtype=dtype))
    B = rows.stop - rows.start
    shb = dataclasses.replace(sh, B=B)
    feats4d = feats[rows].reshape(B, sh.D, sh.S, 1)
    mk = lambda k: None if masks is None else torch.as_tensor(np.ascontiguousarray(masks[k][:, rows]))
    m_q, m_x, m_mf = mk("q"), mk("x"), mk("mf")
    qr = q[rows]
    c = torch.zeros(B, sh.R, dtype=dtype)
    h = torch.zeros(B, sh.R, dtype=dtype)
    hops = []
    for hop in range(sh.H):
        score, dp, a, c, h = multimodal(
            shb, Pm, qr, feats4d, c, h,
            None if m_q is None else m_q[hop],
            None if m_x is None else m_x[hop].reshape(B, sh.D, sh.S, 1),
            None if m_mf is None else m_mf[hop], bf16=bf16)
        hops.append((score, dp, a))
    return hops


def step(sh, params, batch, masks, hop_w, z, bf16=False, F=None, nreg=None, loss="ce", pre_q=None, pre_params=(),
         want_feats=False):
    """z: the leaf's value -- q [B, Q] itself, or (pre_q) the input of the caller's encoder.  Only params["mult"] is
    read; batch gives feats and labels (tokens and lens are the encoder's business)."""
    dtype = torch.float64
    t = lambda a: torch.as_tensor(a).to(dtype)
    mult = t(params["mult"]).clone().requires_grad_(True)
    Pm = _split(mult, mult_specs(sh))
    leaf = t(z).clone().requires_grad_(True)
    q = leaf if pre_q is None else pre_q(leaf)
    assert tuple(q.shape) == (sh.B, 4 * sh.Rq)
    feats = t(batch["feats"]).clone().requires_grad_(bool(want_feats))
    B = sh.B
    parts = [(slice(0, B), None)] if nreg is None else [(slice(b, b + 1), int(nreg[b])) for b in range(B)]
    per_hop = [[] for _ in range(sh.H)]
    for rows, n_b in parts:
        for hop, vals in enumerate(_forward(sh, Pm, q, feats, masks, rows, n_b, bf16, dtype)):
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
    losses = []
    for hop in range(sh.H):
        if ce is not None:
            l = ce(scores[hop])
            losses.append(float(l.detach()))
            if hop_w is not None:
                total = total + float(hop_w[hop]) * l
        else:
            assert hop_w is None or float(hop_w[hop]) == 0.0, "a hop weight on a batch without labels"
    ext = F(scores, dps, atts) if F is not None else None
    if ext is not None:
        total = total + ext
    res = {"logits": np.stack([s.detach().numpy() for s in scores]),
           "dopred": np.stack([d.detach().numpy() for d in dps]),
           "att": np.stack([a.detach().numpy() for a in atts]),
           "losses": np.asarray(losses),
           "ext": 0.0 if ext is None else float(ext.detach())}
    if torch.is_tensor(total) and total.requires_grad:
        total.backward()
    zero = lambda x: (torch.zeros_like(x) if x.grad is None else x.grad).detach().numpy()
    res["g_mult"] = zero(mult)
    res["g_q"] = zero(leaf)
    if want_feats:
        res["g_feats"] = zero(feats)
    res["g_pre"] = [zero(p) for p in pre_params]
    return res
