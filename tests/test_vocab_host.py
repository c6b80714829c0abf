"""Answer vocabularies of any size (K % 4 != 0): what holds without a device.

1. The declarations of rau_logits_pitch in include/rau.h, rau_vqa_amd/_lib.py and bindings/rau.lua, and the
   header's sentence on the logits' pitch at rau_outputs_dev.
2. The CPU side needs nothing at K = 2, 3, 5, 7 (util.SMALL's other sizes): the C++ oracle against the torch
   restatement, tests/bce_ref.py and tests/merge_ref.py against closed forms in fp64, and the numpy statements
   predict.top_answers / set_stats / soft_bce_grad and joint.merged_ce_grad against torch in fp64.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import oracle
from oracle import ref_torch as RT
from rau_vqa_amd import joint, predict
from tests import bce_ref, merge_ref, util

ROOT = Path(__file__).resolve().parent.parent
KS = [2, 3, 5, 7]
GROUPS = ("embed", "rnn", "mult")


def read(*parts):
    return ROOT.joinpath(*parts).read_text()


# ------------------------------------------------------------------------------------------ 1. declarations
def test_header_ctypes_and_lua_declare_rau_logits_pitch():
    from rau_vqa_amd import _lib
    header, lua = read("include", "rau.h"), read("bindings", "rau.lua")
    assert re.search(r"#define RAU_ABI_VERSION 5\b", header)       # additive: the version stays
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    decl = r"\bint rau_logits_pitch\s*\(\s*rau_ctx\s*\*\s*ctx\s*,\s*int32_t\s*\*\s*pitch\s*\)\s*;"
    assert re.search(decl, code) and re.search(decl, cdef)
    assert "rau_logits_pitch" in _lib._SIGS and len(_lib._SIGS["rau_logits_pitch"][1]) == 2
    assert "function RAU:logitsPitch()" in lua
    from rau_vqa_amd.model import RAU
    assert isinstance(RAU.logits_pitch, property)


def test_header_documents_the_pitch_at_rau_outputs_dev():
    header = read("include", "rau.h")
    doc = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header))   # comment lines joined, their leading stars dropped
    at = doc.index("rau_outputs_dev: ctx-owned DEVICE pointers")
    para = doc[at:doc.index("rau_backward_ext: rau_backward_merged with g", at)]
    for phrase in ("*att_pitch = pitch = S rounded up to a multiple of 4", "rau_logits_pitch:",
                   "K rounded up to a multiple of 4", "strides (n*pitch, pitch, 1) with this pitch",
                   "columns K..pitch-1 of every row hold +0", "stays DENSE [H,n,K]"):
        assert phrase in para, phrase
    assert "[H,n,K] DEVICE, dense (NOT pitched), 16-byte aligned" in header
    assert "K < 2" in doc                                      # rau_create's one rule on K


def test_rau_create_no_longer_names_a_multiple_of_four_for_k():
    src = read("rau_vqa_amd", "csrc", "rau_ctx.hip")
    assert "K=%d must be a positive multiple of 4" not in src
    assert re.search(r"NEED\(c\.K >= 2,", src)


# ------------------------------------------------------------------------------------------ 2. the CPU side
def problem(K, seed=123):
    sh = util.shapes(util.SMALL, K=K)
    batch, params, masks = util.make_problem(sh, seed=seed, scale=0.5)
    batch["labels"] = batch["labels"].copy()
    batch["labels"][::3] = K                                   # the last answer
    return sh, batch, params, masks


def answer_set(sh, G=4, seed=7):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, sh.K + 1, (sh.B, G)).astype(np.int32)
    ids[::3, 0] = sh.K
    ids[0, 1] = ids[0, 0]
    ids[1] = 0
    w = (rng.integers(1, 8, (sh.B, G)) / 8).astype(np.float32)
    score = np.minimum(rng.integers(0, 5, (sh.B, G)).astype(np.float32) / np.float32(3), np.float32(1))
    return ids, w, score.astype(np.float32)


@pytest.mark.parametrize("K", KS)
def test_oracle_and_its_restatements_agree(K):
    sh, batch, params, masks = problem(K)
    hop_w = np.array([3.0, 1.0, 2.0], np.float32)
    args = (sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks, hop_w)
    a = oracle.step(*args, dtype=np.float64)
    b = RT.step(*args)
    for k in ("logits", "losses", "dopred") + tuple("g_" + g for g in GROUPS):
        assert util.rel_err(a[k], b[k]) < 1e-9, k
    assert np.array_equal(a["argmax"], b["argmax"])
    # merge_ref without merged terms is the oracle's step; with them it adds joint.merged_ce_grad's term at the logits
    c = merge_ref.step(sh, params, batch, masks, hop_w)
    for g in GROUPS:
        assert util.rel_err(c["g_" + g], a["g_" + g]) < 1e-9, g
    # bce_ref's losses are predict.soft_bce's of its own logits, in fp64
    ids, w, _ = answer_set(sh)
    for answers in (None, (ids, w)):
        r = bce_ref.step(sh, params, batch, masks, hop_w, answers=answers, backward=False)
        si, sw = (batch["labels"][:, None], np.ones((sh.B, 1), np.float32)) if answers is None else answers
        for h in range(sh.H):
            assert abs(predict.soft_bce(r["logits"][h], si, sw, dtype=np.float64)[1] - r["losses"][h]) < 1e-9


@pytest.mark.parametrize("K", KS)
def test_numpy_statements_against_torch(K):
    rng = np.random.default_rng(K)
    H, B = 3, 8
    sh = util.shapes(util.SMALL, K=K)
    lg = rng.normal(size=(H, B, K)).astype(np.float32)
    lg[:, ::3, K - 1] += 2.0                                   # some rows' first maximum is K
    dp = rng.uniform(size=(H, B)).astype(np.float32)
    dp[:, 0], dp[:, 1] = 0.2, 0.9
    ids, w, score = answer_set(sh)
    y = rng.integers(1, K + 1, B).astype(np.int32)
    y[::3] = K
    # top_answers: torch.topk on rows without ties
    for k in (1, K):
        tid, tscore, tconf = predict.top_answers(lg, k)
        tv, ti = torch.topk(torch.as_tensor(lg), k, dim=2)
        assert np.array_equal(tid, ti.numpy() + 1) and np.array_equal(tscore, tv.numpy())
        soft = torch.softmax(torch.as_tensor(lg, dtype=torch.float64), dim=2).numpy()
        assert util.rel_err(tconf, np.take_along_axis(soft, tid - 1, axis=2)) < 1e-6
    assert (predict.top_answers(lg, 1)[0] == K).any()
    # soft_bce_grad: autograd of the summed criterion over the labelled rows, mean over B
    x = torch.as_tensor(lg[0], dtype=torch.float64).requires_grad_(True)
    t = torch.as_tensor(predict.bce_target(ids, w, K).astype(np.float64))
    live = torch.as_tensor((ids > 0).any(axis=1).astype(np.float64)).unsqueeze(1)
    (torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none") * live).sum().div(B).backward()
    assert util.rel_err(predict.soft_bce_grad(lg[0], ids, w), x.grad.numpy()) < 1e-6
    assert not predict.soft_bce_grad(lg[0], ids, w)[1].any()    # the row without entries
    # set_stats: the soft cross-entropy of every row
    s = predict.set_stats(lg, dp, ids, w, score)
    l64 = torch.as_tensor(lg, dtype=torch.float64)
    aw = torch.where(torch.as_tensor(ids) > 0, torch.as_tensor(w, dtype=torch.float64), torch.zeros((), dtype=torch.float64))
    for h in range(H):
        want = float(merge_ref.soft_ce(l64[h], torch.as_tensor(ids).long(), aw, B))
        assert abs(s["loss"][h] - want) < 1e-5 * max(1.0, abs(want))
    # merged_ce_grad: autograd of the two merged rows' cross-entropies with a detached gate
    for truth in ("labels", "set"):
        z = torch.as_tensor(lg, dtype=torch.float64).requires_grad_(True)
        gate = torch.as_tensor(merge_ref.first_fire(dp))
        uni, sel = z.mean(dim=0), (z * gate.unsqueeze(2)).sum(dim=0)
        if truth == "labels":
            ce = lambda r: torch.nn.functional.cross_entropy(r, torch.as_tensor(y).long() - 1)
            kw = {"labels": y}
        else:
            ce = lambda r: merge_ref.soft_ce(r, torch.as_tensor(ids).long(), aw, B)
            kw = {"answers": (ids, w)}
        (0.7 * ce(uni) + 1.3 * ce(sel)).backward()
        got = joint.merged_ce_grad(lg.astype(np.float64), dp, merge_w=[0.7, 1.3], **kw)
        assert util.rel_err(got, z.grad.numpy()) < 1e-9, truth
        assert util.rel_err(joint.merged_ce_grad(lg, dp, merge_w=[0.7, 1.3], **kw), z.grad.numpy()) < 1e-5, truth
