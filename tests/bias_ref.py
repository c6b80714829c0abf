"""Reference for the caller's attention bias (rau_set_att_bias_dev), built from the unchanged oracle.

attbymemory.linear's bias [S] is added to every attention score (SS:287-289) and is shared by the batch, so a bias
PER SAMPLE is one oracle run per sample on a B = 1 shape with bias[b] added to that parameter -- regions_ref's trick,
with that sample's slice of every dropout mask.  Where the bias says -inf the reference writes -1e30: exactly zero
attention in f32 and f64 (exp underflows to 0) and finite gradients.  Region counts, where given, are -1e30 at
s >= n[b] on top.  Outputs are stacked, losses averaged, the parameter gradients taken as (1/B) sum_b g_b; and the
gradient at the bias is that run's gradient at the parameter it was added to: d_bias[b] = g_b[bias slice] / B.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import oracle

from .regions_ref import MASKED, bias_slice


def pattern(B, S, seed=17, edge=None):
    """The tests' bias [B, S] float32: 2 * standard_normal, with rows (cyclically, where B allows) of these kinds --
    0: one finite position only; 1: alternate positions at -inf; 2: -inf from a mask edge that is no multiple of 4;
    3: the last logical position only; 4: a row of zeros; the others keep their random values."""
    b = (2 * np.random.default_rng(seed).standard_normal((B, S))).astype(np.float32)
    edge = (S // 2) | 1 if edge is None else int(edge)
    assert 1 <= edge < S and edge % 4
    one = min(S - 1, 2)
    kinds = {0: lambda r: (r.__setitem__(slice(0, one), -np.inf), r.__setitem__(slice(one + 1, S), -np.inf)),
             1: lambda r: r.__setitem__(slice(1, S, 2), -np.inf),
             2: lambda r: r.__setitem__(slice(edge, S), -np.inf),
             3: lambda r: r.__setitem__(slice(0, S - 1), -np.inf),
             4: lambda r: r.__setitem__(slice(0, S), 0.0)}
    for row in range(min(B, 5)):
        kinds[row](b[row])
    return b


def biased_params(sh, params, bias_b, n_b=None, layout=None, dtype=np.float64):
    """params with attbymemory.linear's bias += bias_b (-inf as -1e30), and -1e30 at s >= n_b where a count is given."""
    sl = bias_slice(sh, layout)
    mult = np.array(params["mult"], dtype=dtype, copy=True)
    add = np.asarray(bias_b, dtype)
    assert add.shape == (sh.S,) and not np.isnan(add).any() and not np.isposinf(add).any()
    row = mult[sl]
    neg = np.isneginf(add)
    row[~neg] += add[~neg]
    row[neg] = MASKED
    if n_b is not None:
        row[int(n_b):] = MASKED
    return {"embed": params["embed"], "rnn": params["rnn"], "mult": mult}


def step(sh, params, batch, masks, hop_w, bias, n=None, dtype=np.float64, layout=None):
    """oracle.step's result for the batch with bias[b, s] added to sample b's attention scores in every hop (and, with
    n, sample b attending to positions [0, n[b]) only), plus d_bias [B, S].
    masks: dict of keep flags (train mode) or None (evaluate mode)."""
    bias = np.asarray(bias)
    assert bias.shape == (sh.B, sh.S)
    if n is not None:
        n = np.asarray(n, np.int64)
        assert n.shape == (sh.B,) and n.min() >= 1 and n.max() <= sh.S
    sl = bias_slice(sh, layout)
    sh1 = dataclasses.replace(sh, B=1)
    outs = []
    for b in range(sh.B):
        mb = None if masks is None else {k: np.ascontiguousarray(v[:, b:b + 1]) for k, v in masks.items()}
        outs.append(oracle.step(sh1, biased_params(sh, params, bias[b], None if n is None else n[b], layout, dtype),
                                batch["feats"][b:b + 1], np.ascontiguousarray(batch["tokens"][:, b:b + 1]),
                                batch["lens"][b:b + 1], batch["labels"][b:b + 1], mb, hop_w, dtype=dtype))
    res = {"losses": np.mean([o["losses"] for o in outs], axis=0),
           "q": np.concatenate([o["q"] for o in outs], axis=0)}
    for k in ("argmax", "logits", "dopred", "att", "att_c", "att_h"):
        res[k] = np.concatenate([o[k] for o in outs], axis=1)
    for k in ("g_embed", "g_rnn", "g_mult"):
        res[k] = np.sum([o[k] for o in outs], axis=0) / sh.B
    res["d_bias"] = np.stack([np.asarray(o["g_mult"])[sl] for o in outs], axis=0) / sh.B
    return res


# ---------------------------------------------------------------------------------------------------------------------
# The same feature on oracle/ref_torch.py, with the bias itself as an fp64 LEAF: for what the flat oracle cannot state
# (bf16 emulation, an attached question or state, an external term F, attention supervision).  tests/state_ref.step's
# construction, run once per sample on a B = 1 shape with that sample's bias row added to attbymemory.linear's bias;
# d_bias is the leaf's gradient.  tests/test_att_bias_host.py holds the two references against each other.
def torch_step(sh, params, batch, masks, hop_w, bias, n=None, bf16=False, c0=None, h0=None, q=None, F=None,
               att_w=None, att_t=None, want_feats=False):
    """sum_h hop_w[h] CE_h + F(scores, dps, atts, cs, hs) + sum_h att_w[h] ATT_h (att_ref's term) with bias [B, S]
    added to the attention scores of every hop (-inf as -1e30), counts n [B] or None, an initial state (c0, h0) or
    zeros, a question state q [B, Q] in the encoder's place or None.  masks None: evaluate mode.  Returns logits,
    dopred, att, c, h [H, B, ..], losses [H], the three gradient groups, d_bias [B, S], d_c0, d_h0 and, where asked
    for, g_q and g_feats."""
    import torch

    from oracle.ref_torch import _split, mult_specs
    from tests import att_ref, state_ref
    dtype = torch.float64
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    flat = {k: t(params[k]).clone().requires_grad_(True) for k in state_ref.GROUPS}
    B = sh.B
    add = np.asarray(bias, np.float64)
    assert add.shape == (B, sh.S) and not np.isnan(add).any() and not np.isposinf(add).any()
    bl = t(np.where(np.isneginf(add), MASKED, add)).clone().requires_grad_(True)
    z = np.zeros((B, sh.R))
    c0l = t(z if c0 is None else c0).clone().requires_grad_(True)
    h0l = t(z if h0 is None else h0).clone().requires_grad_(True)
    ql = None if q is None else t(q).clone().requires_grad_(True)
    feats = t(batch["feats"]).clone().requires_grad_(bool(want_feats))
    Pm = _split(flat["mult"], mult_specs(sh))
    per_hop = [[] for _ in range(sh.H)]
    for b in range(B):
        rows = slice(b, b + 1)
        Pb = dict(Pm)
        Pb["att_mem.b"] = Pm["att_mem.b"] + bl[b]
        qr = state_ref._encoder(sh, flat, batch, masks, rows, dtype) if ql is None else ql[rows]
        hops = state_ref._hops(sh, Pb, qr, feats, c0l[rows], h0l[rows], masks, rows, None if n is None else int(n[b]),
                               bf16, dtype)
        for hop, vals in enumerate(hops):
            per_hop[hop].append(vals)
    scores, dps, atts, cs, hs = ([torch.cat([v[i] for v in per_hop[hop]], 0) for hop in range(sh.H)] for i in range(5))
    y = torch.as_tensor(batch["labels"]).long() - 1
    ce = [torch.nn.functional.cross_entropy(scores[hop], y) for hop in range(sh.H)]
    total = sum(float(hop_w[hop]) * ce[hop] for hop in range(sh.H))
    if F is not None:
        total = total + F(scores, dps, atts, cs, hs)
    if att_w is not None:
        live = torch.ones(B, sh.S, dtype=torch.bool) if n is None else \
            torch.arange(sh.S)[None, :] < torch.as_tensor(np.asarray(n, np.int64))[:, None]
        tt = t(att_t) * live
        for hop in range(sh.H):
            total = total + float(att_w[hop]) * (tt * -torch.log(atts[hop] + att_ref.EPS)).sum() / B
    total.backward()
    stack = lambda v: np.stack([x.detach().numpy() for x in v])
    zero = lambda x: (torch.zeros_like(x) if x.grad is None else x.grad).detach().numpy()
    res = {"logits": stack(scores), "dopred": stack(dps), "att": stack(atts), "c": stack(cs), "h": stack(hs),
           "losses": np.array([float(v.detach()) for v in ce]), "d_bias": zero(bl), "d_c0": zero(c0l), "d_h0": zero(h0l)}
    res["att_c"], res["att_h"] = res["c"], res["h"]
    for k in state_ref.GROUPS:
        res["g_" + k] = zero(flat[k])
    if ql is not None:
        res["g_q"] = zero(ql)
    if want_feats:
        res["g_feats"] = zero(feats)
    return res
