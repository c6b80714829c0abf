"""The mode of the Linear GEMMs (bf16 products, 16- or 32-deep skinny stages) belongs to the context and
the call, not to the calling thread: whatever other contexts, module-level calls or modes the same thread
ran in between, a step computes the bits it computes alone.

Context X: f32, the generic dims of tests/knob_check.py at B = 72 (train mode: above the 64-sample switch,
16-deep stages; R = Rq = 64 makes the 32-deep form eligible in evaluate mode).  Context Y: bf16, the
"bf16" dims at B = 12 (bf16 products, 32-deep stages).  Every comparison is np.array_equal on the raw bits.
"""
import ctypes as C

import numpy as np
import pytest

from rau_vqa_amd import _lib as L
from tests import util

pytestmark = pytest.mark.gpu

X_DIMS = dict(B=72, T=7, V=120, E=200, Rq=64, D=64, S=196, M=128, A=64, R=64, K=1000, H=4)
Y_DIMS = dict(B=12, T=5, V=60, E=64, Rq=64, D=256, S=196, M=256, A=64, R=64, K=200, H=3)
SEED, STEP = 7, 3


def _make(dims, dtype):
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(dims)
    batch, params, _ = util.make_problem(sh, scale=0.2)
    m = RAU(Config(**dims, dtype=dtype))
    m.set_params(params)
    m.training()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    return m


def _begin(m):
    """Fixed inputs (the resident batch), zero gradients, fixed (seed, step); then the forward."""
    m.training()
    m.set_dropout_seed(SEED, STEP)
    m.zero_grads()
    m.forward()


def _finish(m):
    m.backward(np.full(m.cfg.H, float(m.cfg.H), np.float32))
    g = m.get_grads()
    return {"losses": m.losses(), "logits": m.logits(), "g_embed": g["embed"], "g_rnn": g["rnn"],
            "g_mult": g["mult"]}


def _same(got, ref, who):
    for k, r in ref.items():
        assert np.array_equal(got[k].view(np.uint32), r.view(np.uint32)), f"{who}: {k} differs from its run alone"


@pytest.fixture(scope="module")
def ctxs():
    x = _make(X_DIMS, "f32")
    _begin(x)
    x_alone = _finish(x)
    y = _make(Y_DIMS, "bf16")
    _begin(y)
    y_alone = _finish(y)
    for r in (x_alone, y_alone):
        for a in r.values():
            a.setflags(write=False)
    yield x, x_alone, y, y_alone
    x.close()
    y.close()


@pytest.mark.parametrize("first", ["x", "y"])
def test_two_contexts_interleaved_on_one_thread(ctxs, first):
    x, x_alone, y, y_alone = ctxs
    a, b = (x, y) if first == "x" else (y, x)
    _begin(a)
    _begin(b)
    ra = _finish(a)
    rb = _finish(b)
    got = {id(a): ra, id(b): rb}
    _same(got[id(x)], x_alone, "X (f32, 16-deep)")
    _same(got[id(y)], y_alone, "Y (bf16, 32-deep)")


def test_module_level_call_of_another_context_between_forward_and_backward(ctxs):
    from rau_vqa_amd.modules import DevTensor
    x, x_alone, y, _ = ctxs
    _begin(x)
    # lstm_clones[0]:forward on Y: two Linear GEMM pairs in Y's mode (bf16 products, 32-deep stages)
    xin = DevTensor.zeros(y, y.batch_size, y.cfg.E)
    state = DevTensor.zeros(y, y.batch_size, y.cfg.Q)
    out = C.c_void_p()
    L.check(y._lib.rau_deeplstm_forward(y._h, 0, C.c_void_p(xin.ptr), C.c_void_p(state.ptr), C.byref(out)))
    y.sync()
    _same(_finish(x), x_alone, "X (f32, 16-deep)")


def test_one_context_across_modes(ctxs):
    x, x_alone, _, _ = ctxs
    _begin(x)
    _same(_finish(x), x_alone, "X, first train step")
    x.evaluate()        # 72 samples in evaluate mode: chain-bound, 32-deep stages
    x.forward()
    x.sync()
    _begin(x)           # back to train mode, same (seed, step), gradients zeroed
    _same(_finish(x), x_alone, "X, train step after an evaluate-mode forward")
