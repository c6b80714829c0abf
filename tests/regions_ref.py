"""Reference for per-sample region counts (rau_set_regions), built from the unchanged oracle.

The oracle has no mask, but attbymemory.linear's bias [S] is added to every attention score (SS:287-289):
a bias of -1e30 at s >= n gives exactly zero attention there, in f32 and in f64 (exp underflows to 0).  The
bias is shared by the batch, so MIXED counts are one oracle run per sample on a B = 1 shape, with that sample's
slice of every dropout mask and its own bias; outputs are stacked, losses averaged and the gradients taken as
(1/B) sum_b g_b (the criterion averages over the batch, everything else is per sample).
"""
from __future__ import annotations

import dataclasses

import numpy as np

import oracle

MASKED = -1e30


def bias_slice(sh, layout=None) -> slice:
    """Where attbymemory.linear's bias [S] lies in the flat `mult` group: from the device layout
    (RAU.layout("mult"): weight [S, R], then bias) when given, else from the oracle's own layer list."""
    if layout is not None:
        for name, off, rows, cols in layout:
            if name == "attbymemory.linear.bias":
                assert rows * cols == sh.S, (rows, cols)
                return slice(off, off + sh.S)
        raise KeyError("attbymemory.linear.bias")
    from oracle import ref_torch
    off = 0
    for name, o, i in ref_torch.mult_specs(sh):
        if name == "att_mem":
            assert (o, i) == (sh.S, sh.R)
            return slice(off + o * i, off + o * i + o)
        off += o * i + o
    raise KeyError("att_mem")


def masked_params(sh, params, n, layout=None, dtype=np.float64):
    """params with attbymemory.linear's bias at -1e30 for s >= n (one count for the whole batch)."""
    sl = bias_slice(sh, layout)
    mult = np.array(params["mult"], dtype=dtype, copy=True)
    bias = mult[sl]
    bias[int(n):] = MASKED
    return {"embed": params["embed"], "rnn": params["rnn"], "mult": mult}


def step(sh, params, batch, masks, hop_w, n, dtype=np.float64, layout=None):
    """oracle.step's result for the batch with sample b attending to positions [0, n[b]) only.
    masks: dict of keep flags (train mode) or None (evaluate mode)."""
    n = np.asarray(n, np.int64)
    assert n.shape == (sh.B,) and n.min() >= 1 and n.max() <= sh.S
    sh1 = dataclasses.replace(sh, B=1)
    outs = []
    for b in range(sh.B):
        mb = None if masks is None else {k: np.ascontiguousarray(v[:, b:b + 1]) for k, v in masks.items()}
        outs.append(oracle.step(sh1, masked_params(sh, params, n[b], layout, dtype),
                                batch["feats"][b:b + 1], np.ascontiguousarray(batch["tokens"][:, b:b + 1]),
                                batch["lens"][b:b + 1], batch["labels"][b:b + 1], mb, hop_w, dtype=dtype))
    res = {"losses": np.mean([o["losses"] for o in outs], axis=0),
           "q": np.concatenate([o["q"] for o in outs], axis=0)}
    for k in ("argmax", "logits", "dopred", "att", "att_c", "att_h"):
        res[k] = np.concatenate([o[k] for o in outs], axis=1)
    for k in ("g_embed", "g_rnn", "g_mult"):
        res[k] = np.sum([o[k] for o in outs], axis=0) / sh.B
    return res
