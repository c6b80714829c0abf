"""Question state from the caller (rau_set_question_dev, rau_batch_question, rau_question_grad_dev,
rau_get_question_grad) on the host side: the places that declare the calls agree, and tests/question_ref.py with
ref_torch's own encoder in front IS ref_torch's full step -- the cut between the encoder and the hops is where the
oracle has it."""
import ctypes as C
import os
import re

import numpy as np
import torch

from oracle import ref_torch as RT
from rau_vqa_amd import _lib
from tests import question_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "rau_set_question_dev": "int rau_set_question_dev(rau_ctx* ctx, const void* q_dev",
    "rau_batch_question": "int rau_batch_question(rau_ctx* ctx, int* has);",
    "rau_question_grad_dev": "int rau_question_grad_dev(rau_ctx* ctx, const float** dq",
    "rau_get_question_grad": "int rau_get_question_grad(rau_ctx* ctx, float* host",
}
HOP_W = [3, 0.5, 2]


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_has_the_prototypes_at_abi_5():
    header = read("include", "rau.h")
    assert re.search(r"#define RAU_ABI_VERSION 5\b", header)
    for name, proto in PROTOS.items():
        assert proto in header, name
    # the contract the callers rely on is stated where the calls are declared
    section = header[header.index("question state from the caller"):header.index(PROTOS["rau_get_question_grad"])]
    for phrase in ("OVERWRITTEN", "not touched", "detaches", "Q = 4 * Rq", "RAU_FEAT_BF16", "16-byte aligned",
                   "rau_graph_step's key", "no EXTERNAL gradient enters at the question state"):
        assert phrase in section, phrase


def test_lua_and_ctypes_agree_with_the_header():
    lua = read("bindings", "rau.lua")
    cdef = "\n".join(re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S))
    header = re.sub(r"/\*.*?\*/", "", read("include", "rau.h"), flags=re.S)
    for name in PROTOS:
        assert re.search(r"\bint %s\s*\(" % name, cdef), name
        # same number of parameters in the header, the cdef and the ctypes table
        count = lambda text: len(re.search(r"\bint %s\s*\((.*?)\);" % name, text, flags=re.S).group(1).split(","))
        assert count(header) == count(cdef) == len(_lib._SIGS[name][1]), name
        assert _lib._SIGS[name][0] is C.c_int
    for fn, call in (("setQuestionDev", "rau_set_question_dev"), ("questionGrad", "rau_question_grad_dev")):
        assert "function RAU:%s(" % fn in lua and "C.%s(self.h" % call in lua, fn
    assert _lib._SIGS["rau_question_grad_dev"][1] == [C.c_void_p, C.POINTER(C.c_void_p)]


def test_python_has_the_methods():
    model = read("rau_vqa_amd", "model.py")
    for fn in ("set_question", "clear_question", "batch_question", "question_grad", "question_grad_tensor"):
        assert "def %s(" % fn in model, fn
    assert re.search(r"def set_batch_dev\([^)]*question=None", model)
    autograd = read("rau_vqa_amd", "autograd.py")
    assert re.search(r"def step\([^)]*feats=None, question=None\)", autograd)
    assert "question_grad_tensor()" in autograd and "torch.nn.GRU" in autograd


def test_the_library_exports_the_calls_and_checks_null():
    lib = _lib.lib()
    assert lib.rau_abi_version() == 5
    assert lib.rau_set_question_dev(None, None, 0) == -1 and b"null" in lib.rau_last_error()
    assert lib.rau_batch_question(None, None) == -1
    assert lib.rau_question_grad_dev(None, None) == -1
    assert lib.rau_get_question_grad(None, None) == -1


def test_the_cut_is_where_the_oracle_has_it():
    """question_ref.step with pre_q = ref_torch's embed + deep_lstm + length select reproduces ref_torch's full-step
    gradients of all three groups: fp64 against fp64, 1e-10."""
    sh = util.shapes(util.SMALL)
    batch, params, masks = util.make_problem(sh, scale=0.5)
    full = RT.step(sh, params, batch["feats"], batch["tokens"], batch["lens"], batch["labels"], masks, HOP_W)
    emb = torch.as_tensor(params["embed"]).double().requires_grad_(True)
    rnn = torch.as_tensor(params["rnn"]).double().requires_grad_(True)
    pre_q = lambda z: question_ref.encoder_q(sh, emb, rnn, batch, masks) + 0.0 * z
    ref = question_ref.step(sh, params, batch, masks, HOP_W, np.zeros((sh.B, 4 * sh.Rq)), pre_q=pre_q,
                            pre_params=(emb, rnn))
    assert np.max(np.abs(full["g_embed"])) > 0 and np.max(np.abs(full["g_rnn"])) > 0
    for got, want, what in ((ref["g_pre"][0], full["g_embed"], "g_embed"), (ref["g_pre"][1], full["g_rnn"], "g_rnn"),
                            (ref["g_mult"], full["g_mult"], "g_mult"), (ref["logits"], full["logits"], "logits"),
                            (ref["losses"], full["losses"], "losses")):
        e = util.rel_err(got, want)
        print(f"{what}: rel_err {e:.2e}")
        assert e < 1e-10, what
    # ... and the same step from the leaf q = the encoder's output: the gradient at the leaf, pushed through the
    # encoder by hand, is the encoder's gradient (what a caller's q.backward(dq) does)
    q = question_ref.encoder_q(sh, emb, rnn, batch, masks)
    assert util.rel_err(q.detach().numpy(), full["q"]) < 1e-12
    leaf = question_ref.step(sh, params, batch, masks, HOP_W, q.detach().numpy())
    emb.grad = rnn.grad = None
    q.backward(torch.as_tensor(leaf["g_q"]))
    assert util.rel_err(emb.grad.numpy(), full["g_embed"]) < 1e-10
    assert util.rel_err(rnn.grad.numpy(), full["g_rnn"]) < 1e-10
    assert util.rel_err(leaf["g_mult"], full["g_mult"]) < 1e-10
