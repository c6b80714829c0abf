"""Reference for the per-position L2 normalisation of feature maps (rau_set_feat_norm), built on the unchanged oracle.

The normalisation is torch.nn.functional.normalize(x, p=2, dim=channel, eps=eps) in float64, composed in front of the
existing oracle calls: step() hands oracle.step the float64-normalised maps; feat_step() hands tests/featgrad_ref.py's
step the normalisation as its differentiable `pre` stage, so g_feats is the gradient at the RAW maps (at the table
[N,D,S] where image_of is given).
"""
from __future__ import annotations

import numpy as np
import torch

import oracle
from tests import featgrad_ref


def normalize64(feats, eps):
    """(xn, nrm) of maps [n, D, S] in float64: F.normalize over the channel axis, and the norms [n, S]."""
    x = torch.as_tensor(np.asarray(feats, np.float64))
    xn = torch.nn.functional.normalize(x, p=2.0, dim=1, eps=float(eps))
    return xn.numpy(), torch.sqrt((x * x).sum(1)).numpy()


def normalize_grad64(feats, g, eps):
    """The gradient at the maps of sum(g * normalize(feats)), by float64 autograd through F.normalize."""
    x = torch.as_tensor(np.asarray(feats, np.float64)).clone().requires_grad_(True)
    xn = torch.nn.functional.normalize(x, p=2.0, dim=1, eps=float(eps))
    (xn * torch.as_tensor(np.asarray(g, np.float64))).sum().backward()
    return x.grad.numpy()


def step(sh, params, batch, masks, hop_w, eps, dtype=np.float64):
    """oracle.step on the float64-normalised maps of the batch."""
    xn, _ = normalize64(batch["feats"], eps)
    return oracle.step(sh, params, xn, batch["tokens"], batch["lens"], batch["labels"], masks, hop_w, dtype=dtype)


def feat_step(sh, params, batch, masks, hop_w, eps, image_of=None):
    """featgrad_ref.step with the normalisation as the stage in front: g_feats is the gradient at the raw maps
    batch["feats"] -- [B, D, S], or with image_of [B] the table [N, D, S] the samples share."""
    idx = None if image_of is None else torch.as_tensor(np.asarray(image_of)).long()

    def pre(x):
        xn = torch.nn.functional.normalize(x, p=2.0, dim=1, eps=float(eps))
        return xn if idx is None else xn[idx]
    return featgrad_ref.step(sh, params, batch, masks, hop_w, pre=pre)
