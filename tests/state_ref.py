"""Reference for the open hop recurrence (rau_set_state_dev, rau_backward_state), built on the unchanged
oracle/ref_torch.py.

tests/ext_ref.step restated with the initial state (c0, h0) [B, R] of the hop chain as fp64 leaves: ref_torch's own
multimodal, deep_lstm, _drop, _split and specs, with a hop loop of its own (att_ref._forward starts from zeros).  The
objective is ext_ref's with the hop states among F's arguments:

    sum_h hop_w[h] * CE_h  +  F(scores, dps, atts, cs, hs)

F is a Python callable on five lists of H fp64 tensors WITH their graphs: scores [B, K], dps [B], atts [B, S],
cs [B, R], hs [B, R] (c' and h' of every hop); it returns a scalar tensor, None is no such term.  A batch without labels
has no criterion: hop_w must then be None or zeros.  masks None: evaluate mode.  With region counts the forward runs
once per sample on a B = 1 shape (the method of tests/regions_ref.py, through att_ref.MASKED), each on its rows of the
same leaves.  q: a question state [B, Q] that stands where the encoder's output would (rau_set_question_dev), a leaf
as well; want_feats: the maps are a leaf too.

step() returns the outputs, c / h of every hop [H, B, R], the three gradient groups, d_c0, d_h0 [B, R] and, where
asked for, g_q and g_feats.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle.ref_torch import _drop, _split, deep_lstm, mult_specs, multimodal, rnn_specs
from tests import att_ref

GROUPS = ("embed", "rnn", "mult")


def _encoder(sh, flat, batch, masks, rows, dtype):
    """ref_torch._step's encoder loop for the samples `rows`: q [B, Q]."""
    Emb = flat["embed"].view(sh.V, sh.E)
    Pr = _split(flat["rnn"], rnn_specs(sh))
    B = rows.stop - rows.start
    shb = dataclasses.replace(sh, B=B)
    tokens = torch.as_tensor(np.ascontiguousarray(batch["tokens"][:, rows])).long()
    lens = torch.as_tensor(batch["lens"][rows]).long()
    mk = lambda k: None if masks is None else torch.as_tensor(np.ascontiguousarray(masks[k][:, rows]))
    m_we, m_rnn = mk("we"), mk("rnn")
    state = torch.zeros(B, 4 * sh.Rq, dtype=dtype)
    q = torch.zeros(B, 4 * sh.Rq, dtype=dtype)
    for tt in range(1, int(lens.max()) + 1):
        we = torch.tanh(_drop(Emb[tokens[tt - 1] - 1], None if m_we is None else m_we[tt - 1], sh.p_we))
        state = deep_lstm(shb, Pr, we, state, None if m_rnn is None else m_rnn[tt - 1])
        q = torch.where((lens == tt).unsqueeze(1), state, q)
    return q


def _hops(sh, Pm, q, feats, c, h, masks, rows, n_b, bf16, dtype):
    """The hop loop from (c, h) for the samples `rows`: per hop (score, do_pred, attprob, c', h')."""
    Pm = dict(Pm)
    if n_b is not None:
        live = torch.arange(sh.S) < int(n_b)
        Pm["att_mem.b"] = torch.where(live, Pm["att_mem.b"], torch.full((), att_ref.MASKED, dtype=dtype))
    B = rows.stop - rows.start
    shb = dataclasses.replace(sh, B=B)
    feats4d = feats[rows].reshape(B, sh.D, sh.S, 1)
    mk = lambda k: None if masks is None else torch.as_tensor(np.ascontiguousarray(masks[k][:, rows]))
    m_q, m_x, m_mf = mk("q"), mk("x"), mk("mf")
    out = []
    for hop in range(sh.H):
        score, dp, a, c, h = multimodal(
            shb, Pm, q, feats4d, c, h,
            None if m_q is None else m_q[hop],
            None if m_x is None else m_x[hop].reshape(B, sh.D, sh.S, 1),
            None if m_mf is None else m_mf[hop], bf16=bf16)
        out.append((score, dp, a, c, h))
    return out


def step(sh, params, batch, masks, hop_w, c0, h0, F=None, nreg=None, bf16=False, q=None, want_feats=False,
         backward=True):
    dtype = torch.float64
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    flat = {k: t(params[k]).clone().requires_grad_(backward) for k in GROUPS}
    Pm = _split(flat["mult"], mult_specs(sh))
    B = sh.B
    c0l = t(c0).clone().requires_grad_(backward)
    h0l = t(h0).clone().requires_grad_(backward)
    assert tuple(c0l.shape) == tuple(h0l.shape) == (B, sh.R)
    ql = None if q is None else t(q).clone().requires_grad_(backward)
    feats = t(batch["feats"]).clone().requires_grad_(bool(want_feats and backward))
    parts = [(slice(0, B), None)] if nreg is None else [(slice(b, b + 1), int(nreg[b])) for b in range(B)]
    per_hop = [[] for _ in range(sh.H)]
    for rows, n_b in parts:
        qr = _encoder(sh, flat, batch, masks, rows, dtype) if ql is None else ql[rows]
        for hop, vals in enumerate(_hops(sh, Pm, qr, feats, c0l[rows], h0l[rows], masks, rows, n_b, bf16, dtype)):
            per_hop[hop].append(vals)
    cat = lambda hop, i: (per_hop[hop][0][i] if len(parts) == 1 else torch.cat([v[i] for v in per_hop[hop]], 0))
    scores, dps, atts, cs, hs = ([cat(hop, i) for hop in range(sh.H)] for i in range(5))

    total = 0.0
    if batch.get("labels") is not None:
        y = torch.as_tensor(batch["labels"]).long() - 1
        for hop in range(sh.H):
            if hop_w is not None:
                total = total + float(hop_w[hop]) * torch.nn.functional.cross_entropy(scores[hop], y)
    else:
        assert hop_w is None or not np.any(np.asarray(hop_w)), "a hop weight on a batch without labels"
    ext = F(scores, dps, atts, cs, hs) if F is not None else None
    if ext is not None:
        total = total + ext
    stack = lambda v: np.stack([x.detach().numpy() for x in v])
    res = {"logits": stack(scores), "dopred": stack(dps), "att": stack(atts), "c": stack(cs), "h": stack(hs),
           "ext": 0.0 if ext is None else float(ext.detach())}
    if backward:
        if torch.is_tensor(total) and total.requires_grad:
            total.backward()
        zero = lambda x: (torch.zeros_like(x) if x.grad is None else x.grad).detach().numpy()
        for k in GROUPS:
            res["g_" + k] = zero(flat[k])
        res["d_c0"], res["d_h0"] = zero(c0l), zero(h0l)
        if ql is not None:
            res["g_q"] = zero(ql)
        if want_feats:
            res["g_feats"] = zero(feats)
    return res


def linear_F(G_l=None, G_d=None, G_a=None, G_h=None, G_c_last=None):
    """ext_ref.linear_F's construction extended to the states: F = sum_h <G_l[h], logits_h> + <G_d[h], dopred_h> +
    <G_a[h], att_h> + <G_h[h], h'_h>  +  <G_c_last, c'_{H-1}> for fixed arrays (None: no such sum); its gradients at
    the outputs and states are the G themselves."""
    def F(scores, dps, atts, cs, hs):
        tot = 0.0
        for G, outs in ((G_l, scores), (G_d, dps), (G_a, atts), (G_h, hs)):
            if G is not None:
                for h, o in enumerate(outs):
                    tot = tot + (torch.as_tensor(np.asarray(G[h], np.float64)) * o).sum()
        if G_c_last is not None:
            tot = tot + (torch.as_tensor(np.asarray(G_c_last, np.float64)) * cs[-1]).sum()
        return tot
    return F
