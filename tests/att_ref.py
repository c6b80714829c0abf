"""Reference for attention supervision (rau_backward_att), built on the unchanged oracle/ref_torch.py.

ref_torch._step restated (as tests/test_gpu_select.py::oracle_step restates it) on ref_torch's own multimodal,
deep_lstm, _drop, _split and specs -- multimodal's third return value is the attention WITH its graph -- in fp64
with explicit masks, and with

    sum_h att_w[h] * ATT_h,    ATT_h = (1/B) sum_b sum_{s < n_reg[b]} t[b,s] * (-log(a[h,b,s] + 1e-12))

added to sum_h hop_w[h] * CE_h.  With region counts the step runs once per sample on a B = 1 shape, with that
sample's slice of every dropout mask and attbymemory.linear's bias at -1e30 behind its count (the method of
tests/regions_ref.py: the bias is shared by a batch, so mixed counts need one run per sample), each sample's loss
scaled by 1/B; everything hangs on ONE set of leaf parameters, so one backward gives (1/B) sum_b g_b.

targets() builds the seeded target maps of the tests and states the condition they must meet.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle.ref_torch import _drop, _split, deep_lstm, mult_specs, multimodal, rnn_specs

EPS = 1e-12
MASKED = -1e30
A_MIN = 1e-4          # the condition on the inputs: every a >= A_MIN where t > 0 (fp64 oracle)
GROUPS = ("embed", "rnn", "mult")


def _forward(sh, flat, batch, masks, rows, n_b, bf16, dtype):
    """The encoder and the hops for the samples `rows` (a slice) on a shape of that many samples; n_b: the one
    region count of those samples or None.  Returns per hop (score, do_pred, attprob, c, h) and q."""
    t = lambda a: torch.as_tensor(a).to(dtype)
    Emb = flat["embed"].view(sh.V, sh.E)
    Pr = _split(flat["rnn"], rnn_specs(sh))
    Pm = dict(_split(flat["mult"], mult_specs(sh)))
    if n_b is not None:
        live = torch.arange(sh.S) < int(n_b)
        Pm["att_mem.b"] = torch.where(live, Pm["att_mem.b"], torch.full((), MASKED, dtype=dtype))
    B = rows.stop - rows.start
    shb = dataclasses.replace(sh, B=B)
    feats4d = t(batch["feats"][rows]).reshape(B, sh.D, sh.S, 1)
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
        hops.append((score, dp, a, c, h))
    return hops, q


def step(sh, params, batch, masks, hop_w, att_w=None, t=None, nreg=None, bf16=False, backward=True):
    """One step with the attention term.  att_w None or t None: no term (ref_torch.step's loss).  masks None:
    evaluate mode.  Returns ref_torch.step's keys plus ``att_losses`` [H] (ATT_h, unweighted)."""
    dtype = torch.float64
    flat = {k: torch.as_tensor(params[k]).to(dtype).clone().requires_grad_(backward) for k in GROUPS}
    B = sh.B
    y = torch.as_tensor(batch["labels"]).long() - 1
    tt = None if t is None else torch.as_tensor(np.asarray(t, np.float64))
    if att_w is None:
        att_w = [0.0] * sh.H
    parts = [(slice(0, B), None)] if nreg is None else [(slice(b, b + 1), int(nreg[b])) for b in range(B)]
    keys = ("logits", "dopred", "att", "att_c", "att_h")
    out = {k: [[] for _ in range(sh.H)] for k in keys}
    qs = []
    ce = [0.0] * sh.H
    att = [0.0] * sh.H
    for rows, n_b in parts:
        hops, q = _forward(sh, flat, batch, masks, rows, n_b, bf16, dtype)
        qs.append(q.detach())
        for hop, vals in enumerate(hops):
            score, _dp, a, _c, _h = vals
            for k, v in zip(keys, vals):
                out[k][hop].append(v.detach())
            ce[hop] = ce[hop] + torch.nn.functional.cross_entropy(score, y[rows], reduction="sum") / B
            if tt is not None:
                tb = tt[rows]
                if n_b is not None:
                    tb = tb * (torch.arange(sh.S) < n_b)
                att[hop] = att[hop] + (tb * -torch.log(a + EPS)).sum() / B
    res = {k: torch.stack([torch.cat(v, 0) for v in out[k]]).numpy() for k in keys}
    res["q"] = torch.cat(qs, 0).numpy()
    res["argmax"] = np.argmax(res["logits"], axis=-1) + 1
    res["losses"] = np.array([float(v.detach()) for v in ce])
    res["att_losses"] = np.array([float(v.detach()) if torch.is_tensor(v) else v for v in att])
    if backward:
        total = sum(float(hop_w[h]) * ce[h] + float(att_w[h]) * att[h] for h in range(sh.H))
        total.backward()
        for k in GROUPS:
            g = flat[k].grad
            res["g_" + k] = (torch.zeros_like(flat[k]) if g is None else g).numpy()
    return res


def targets(att, nreg=None, seed=3):
    """Seeded target maps [B, S] for a problem whose fp64 oracle attention is att [H, B, S], mixing the four
    kinds of row: normalised smooth rows, a one-hot row (row 0, at hop 0's first maximum), an un-normalised row
    (row 2) and two all-zero rows (rows 1 and the last one; B = 5 at least).  A target is only placed where every
    hop's attention is at least 10 * A_MIN (and below the count), so that the condition  a >= A_MIN where t > 0
    holds with room; check() asserts it.  Behind a count the maps keep their smooth values: they are to be ignored."""
    att = np.asarray(att, np.float64)
    _H, B, S = att.shape
    assert B >= 5
    rng = np.random.default_rng(seed)
    pos = np.arange(S)[None, :]
    centre = rng.uniform(0, S, size=(B, 1))
    width = rng.uniform(max(S / 8, 1.0), max(S / 3, 2.0), size=(B, 1))
    t = np.exp(-0.5 * ((pos - centre) / width) ** 2) + 0.05
    n = np.full(B, S) if nreg is None else np.asarray(nreg)
    live = pos < n[:, None]
    ok = (att.min(axis=0) >= 10 * A_MIN) & live
    t = np.where(ok | ~live, t, 0.0)
    t /= np.where(live, t, 0.0).sum(axis=1, keepdims=True)      # a distribution over the live positions
    t[0] = 0.0
    t[0, int(np.argmax(np.where(live[0], att[0, 0], -1.0)))] = 1.0
    t[2] *= 3.7
    t[1] = 0.0
    t[B - 1] = 0.0
    return np.ascontiguousarray(t, np.float32)


def check(att, t, nreg=None):
    """The condition on the inputs: in the fp64 oracle every a >= A_MIN where t > 0 (below the counts)."""
    att = np.asarray(att, np.float64)
    S = att.shape[-1]
    n = np.full(att.shape[1], S) if nreg is None else np.asarray(nreg)
    on = (np.asarray(t) > 0) & (np.arange(S)[None, :] < n[:, None])
    assert on.any()
    assert att[:, on].min() >= A_MIN, float(att[:, on].min())
    kinds = on.sum(axis=1)
    assert (kinds == 0).sum() >= 2 and (kinds == 1).sum() >= 1 and (kinds > 1).sum() >= 2
    return True
