"""rau_set_batch_size: one context runs batches smaller than the B it was created for, and then behaves
BIT FOR BIT like a context created at that size in the same process (include/rau.h).

Every comparison below is np.array_equal between a context of capacity `cap` resized to n and a fresh
context with B = n holding the same parameters, dropout seed and mode; the oracle test pins that "equal
to a fresh context" is also correct.  The resized context always runs a step of non-zero data at another
size first, so the memory the dense layouts then move over is dirty.  Fresh-context results are computed
once per (widths, n, dtype) and shared by the tests that need them."""
import numpy as np
import pytest

from rau_vqa_amd import feat16
from rau_vqa_amd import _lib as L
from tests import test_gpu_parity, util
from tests.test_gpu_graph import _mk as graph_model   # the graph tests' own model construction

pytestmark = pytest.mark.gpu

# small widths (tests/util.SMALL's) with room for the reference's batch sizes
W = dict(T=6, V=50, E=8, Rq=16, D=24, S=12, M=40, A=20, R=16, K=12, H=3)
W49 = dict(T=5, V=40, E=8, Rq=16, D=24, S=49, M=40, A=20, R=16, K=12, H=3)      # 7x7 maps: pitch 52
ERR_INVALID, ERR_STATE = -1, -3
KEYS = ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H", "p_we", "p_rnn", "p_q", "p_x", "p_mf")


def narrow(a, ft):
    """f32 maps -> elements of ft (f16: float16, bf16: uint16 bits), round to nearest even"""
    out = np.empty(np.shape(a), feat16.dtype_of(ft))
    feat16.store(out, a)
    return out


def model(widths, B, params, dtype="f32"):
    from rau_vqa_amd.model import RAU, Config
    sh = util.shapes(widths, B=B)
    m = RAU(Config(**{k: getattr(sh, k) for k in KEYS}, dtype=dtype))
    m.set_params(params)
    return m


def problem(widths, n, seed=123, lens="ragged", scale=0.3):
    """batch of n rows, parameters (independent of n), an MC list [n, 4]"""
    batch, params, _ = util.make_problem(util.shapes(widths, B=n), seed=seed, lens=lens, scale=scale)
    mc = np.random.default_rng(seed).integers(0, widths["K"] + 1, (n, 4)).astype(np.int32)
    return batch, params, mc


def train_step(m, batch, hop_w, step_t=0, update=True, stats=True):
    m.training()
    m.set_dropout_seed(7, 3 + step_t)
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.zero_grads()
    m.forward()
    out = {"t_" + k: v for k, v in m.outputs().items()}
    if stats:
        s = m.step_stats()
        out.update({"s_" + k: np.asarray(v) for k, v in s.items()})
    m.backward(hop_w)
    out.update({"g_" + k: v for k, v in m.get_grads().items()})
    if update:
        out["norms"] = m.update(step_t=step_t, noise_seed=5)
        out.update({"p_" + k: v for k, v in m.get_params().items()})
    return out


def eval_step(m, batch, mc):
    m.evaluate()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.forward()
    out = {"e_" + k: v for k, v in m.outputs().items()}
    out["oe"], out["mc"] = m.predict(mc)
    out["m_pred"], out["m_att"] = m.merged()
    s = m.step_stats()
    out.update({"es_" + k: np.asarray(v) for k, v in s.items()})
    return out


def sequence(m, widths, n, train=True):
    batch, _, mc = problem(widths, n)
    hop_w = np.full(widths["H"], float(widths["H"]), np.float32)
    out = train_step(m, batch, hop_w) if train else {}
    out.update(eval_step(m, batch, mc))
    return out


def same(a, b, what=""):
    assert sorted(a) == sorted(b)
    bad = [k for k in a if not (a[k].shape == b[k].shape and np.array_equal(a[k], b[k]))]
    assert not bad, f"{what}: differ from the fresh context: {bad}"


_fresh = {}


def fresh(widths, n, dtype="f32", train=True):
    key = (tuple(sorted(widths.items())), n, dtype, train)
    if key not in _fresh:
        _, params, _ = problem(widths, n)
        m = model(widths, n, params, dtype)
        _fresh[key] = sequence(m, widths, n, train)
        m.close()
    return _fresh[key]


def resized(widths, cap, n, dtype="f32", dirty=True):
    """a context of `cap` rows that has run a step of non-zero data at another size, now at n rows"""
    _, params, _ = problem(widths, n)
    m = model(widths, cap, params, dtype)
    assert (m.batch_size, m.capacity) == (cap, cap)
    other = cap if n != cap else max(1, cap // 2 - 1)
    if other != cap:
        m.set_batch_size(other)
    if dirty:
        b, _, mc = problem(widths, other, seed=9)
        if dirty == "eval":
            eval_step(m, b, mc)
        else:
            train_step(m, b, np.ones(widths["H"], np.float32), update=False)   # (no update: the Adam state stays fresh)
    m.set_batch_size(n)
    n_now, c_now = L.C.c_int32(), L.C.c_int32()
    L.check(m._lib.rau_batch_size(m._h, L.C.byref(n_now), L.C.byref(c_now)))
    assert (n_now.value, c_now.value, m.batch_size) == (n, cap, n)
    return m


# ---- 1. resized == fresh: both policy thresholds (32 | 33, 64 | 65) and the reference's sizes
@pytest.mark.parametrize("n", [1, 32, 33, 64, 65, 83, 96, 100])
def test_resized_equals_fresh(n):
    m = resized(W, 100, n)
    same(sequence(m, W, n), fresh(W, n), f"100 -> {n}")
    m.close()


def test_resized_equals_fresh_bf16():
    m = resized(W, 100, 83, "bf16")
    same(sequence(m, W, 83), fresh(W, 83, "bf16"), "bf16 100 -> 83")
    m.close()


def test_resized_equals_fresh_real_widths_eval():
    real = dict(T=10, V=500, E=200, Rq=512, D=512, S=196, M=512, A=256, R=512, K=1000, H=8)
    m = resized(real, 100, 83, dirty="eval")
    same(sequence(m, real, 83, train=False), fresh(real, 83, train=False), "real widths 100 -> 83")
    m.close()


def test_resized_equals_fresh_d2048_bf16():
    res = dict(T=6, V=200, E=200, Rq=512, D=2048, S=196, M=512, A=256, R=512, K=1000, H=8)
    m = resized(res, 80, 32, "bf16")
    same(sequence(m, res, 32), fresh(res, 32, "bf16"), "D = 2048 bf16 80 -> 32")
    m.close()


# ---- 2. against the oracle, with the helpers and bars of tests/test_gpu_parity unchanged
@pytest.mark.parametrize("n", [83, 5])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_resized_context_against_the_oracle(n, mode, monkeypatch):
    def run_gpu(sh, batch, params, masks, hop_w, mode="train"):
        m = resized(W, 100, sh.B)
        m.set_params(params)
        if mode == "train":
            m.training()
            m.set_masks(masks)
        else:
            m.evaluate()
        m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
        m.zero_grads()
        m.forward()
        out = m.outputs()
        m.backward(hop_w)
        g = m.get_grads()
        out.update({"g_embed": g["embed"], "g_rnn": g["rnn"], "g_mult": g["mult"]})
        layouts = {k: m.layout(k) for k in ("embed", "rnn", "mult")}
        m.close()
        return out, layouts
    monkeypatch.setattr(test_gpu_parity, "run_gpu", run_gpu)
    test_gpu_parity.check(util.shapes(W, B=n), mode=mode, scale=0.5)


# ---- 3. there and back: an evaluation excursion leaves training exactly where it was
def test_there_and_back():
    b100, params, _ = problem(W, 100)
    b100b, _, _ = problem(W, 100, seed=77)
    b83, _, mc = problem(W, 83, seed=31)
    hop_w = np.full(W["H"], float(W["H"]), np.float32)
    a, b = model(W, 100, params), model(W, 100, params)
    ra = [train_step(a, b100, hop_w, 0)]
    a.set_batch_size(83)
    eval_step(a, b83, mc)
    a.set_batch_size(100)
    ra += [train_step(a, b100b, hop_w, 1), train_step(a, b100, hop_w, 2)]
    rb = [train_step(b, b100, hop_w, 0), train_step(b, b100b, hop_w, 1), train_step(b, b100, hop_w, 2)]
    for k, (x, y) in enumerate(zip(ra, rb)):
        same(x, y, f"training step {k}")
    a.close()
    b.close()


# ---- 4. stale memory: 7x7 maps (pad columns), initial-state rows in use (short and empty questions)
@pytest.mark.parametrize("first,then", [(8, 5), (5, 8)])
@pytest.mark.parametrize("lens", ["ragged", "short"])
def test_stale_memory(first, then, lens):
    def lens_of(n):
        return "ragged" if lens == "ragged" else (np.arange(n, dtype=np.int32) % 3)   # 0, 1, 2, 0, ...
    hop_w = np.ones(W49["H"], np.float32)
    bt, params, mc = problem(W49, then, lens=lens_of(then))
    bf, _, mcf = problem(W49, first, seed=5, lens="full")
    f = model(W49, then, params)
    want = train_step(f, bt, hop_w)
    want.update(eval_step(f, bt, mc))
    f.close()
    m = model(W49, 8, params)
    m.set_batch_size(first)
    train_step(m, bf, hop_w, update=False)
    eval_step(m, bf, mcf)
    m.set_batch_size(then)
    got = train_step(m, bt, hop_w)
    got.update(eval_step(m, bt, mc))
    same(got, want, f"{first} -> {then}")
    m.close()


# ---- 5. every batch path at reduced size equals the plain f32 batch at that size
def _plain(widths, n, batch, params, mc, hop_w):
    f = model(widths, n, params)
    want = train_step(f, batch, hop_w, update=False)
    want.update(eval_step(f, batch, mc))
    f.close()
    return want


def _both(m, hand_over, mc, hop_w):
    """train step (no update) + evaluate step with the batch handed over by `hand_over(m)`"""
    m.training()
    m.set_dropout_seed(7, 3)
    hand_over(m)
    m.zero_grads()
    m.forward()
    out = {"t_" + k: v for k, v in m.outputs().items()}
    out.update({"s_" + k: np.asarray(v) for k, v in m.step_stats().items()})
    m.backward(hop_w)
    out.update({"g_" + k: v for k, v in m.get_grads().items()})
    m.evaluate()
    hand_over(m)
    m.forward()
    out.update({"e_" + k: v for k, v in m.outputs().items()})
    out["oe"], out["mc"] = m.predict(mc)
    out["m_pred"], out["m_att"] = m.merged()
    out.update({"es_" + k: np.asarray(v) for k, v in m.step_stats().items()})
    return out


@pytest.mark.parametrize("widths,cap,n", [(W, 100, 83), (W49, 8, 5)], ids=["s12-100-83", "s49-8-5"])
def test_every_batch_path_at_reduced_size(widths, cap, n):
    batch, params, mc = problem(widths, n)
    hop_w = np.ones(widths["H"], np.float32)
    y, x, xl = batch["labels"], batch["tokens"], batch["lens"]
    nimg = max(1, n // 3)
    image_of = (np.arange(n) * 7 % nimg).astype(np.int32)
    image_of[:nimg] = np.arange(nimg)
    for ft in ("f16", "bf16", "f32"):
        # maps that are exactly representable in ft, so the plain f32 batch of the widened values is the reference
        table = feat16.widen(narrow(batch["feats"][:nimg], ft), ft) if ft != "f32" else batch["feats"][:nimg]
        full = table[image_of]
        typed = lambda a: a if ft == "f32" else narrow(a, ft)
        want = _plain(widths, n, dict(batch, feats=full), params, mc, hop_w)
        m = resized(widths, cap, cap)                           # at capacity, dirty
        m.bank_create(nimg + 2, ft)
        m.bank_put(1, typed(table), ft)                         # filled BEFORE the resize
        m.set_batch_size(n)
        assert m.bank_info()["rows_filled"] == nimg
        rows = (np.arange(nimg) + 1).astype(np.int32)
        paths = {
            "typed": lambda r: r.set_batch(typed(full), x, xl, y, feat_type=ft),
            "table": lambda r: r.set_batch(typed(table), x, xl, y, feat_type=ft, image_of=image_of),
            "bank": lambda r: r.set_batch(None, x, xl, y, bank_rows=rows, image_of=image_of),
        }

        def slot_copy(r, s=[0]):
            s[0] ^= 1
            r.set_batch_async(s[0], typed(full), x, xl, y, feat_type=ft)
            r.use_batch(s[0])

        def slot_in_place(r, s=[0]):
            s[0] ^= 1
            v = r.batch_slot(s[0], feat_type=ft)
            assert v["feats"].shape == (n, widths["D"], widths["S"]) and v["tokens"].shape == (widths["T"], n)
            assert v["lens"].shape == (n,) and v["labels"].shape == (n,)
            v["feats"][...] = typed(full)
            v["tokens"][...] = x
            v["lens"][...] = xl
            v["labels"][...] = y
            r.set_batch_async(s[0], has_labels=True, feat_type=ft)
            r.use_batch(s[0])

        def slot_bank(r, s=[0]):
            s[0] ^= 1
            r.set_batch_async(s[0], None, x, xl, y, bank_rows=rows, image_of=image_of)
            r.use_batch(s[0])
        paths.update({"slot_copy": slot_copy, "slot_in_place": slot_in_place, "slot_bank": slot_bank})
        for name, hand_over in paths.items():
            same(_both(m, hand_over, mc, hop_w), want, f"{ft} {name} at {n} of {cap}")
        m.close()


# ---- 6. module level at n == step level at n (the comparison tests/test_gpu_modules.py makes)
def test_module_level_calls_at_reduced_size():
    import torch
    from rau_vqa_amd import modules
    from tests.test_gpu_modules import cuda
    n = 5
    batch, params, _ = problem(util.SMALL, n, scale=0.5)
    hop_w = np.ones(util.SMALL["H"], np.float32)
    m = resized(util.SMALL, 8, n)
    m.set_params(params)
    m.training()
    m.set_dropout_seed(77, 5)
    m.zero_grads()
    losses, answers = modules.feval(m, cuda(batch["feats"]), cuda(batch["tokens"], torch.int32),
                                    cuda(batch["lens"], torch.int32), cuda(batch["labels"], torch.int32), hop_w)
    m.sync()
    g_mod = m.get_grads()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.set_dropout_seed(77, 5)
    m.zero_grads()
    m.forward()
    m.backward(hop_w)
    g_step = m.get_grads()
    assert answers.shape[-1] == n and m.argmax().shape == (util.SMALL["H"], n)
    assert util.rel_err(losses.numpy(), m.losses()) < 1e-5
    for k in g_step:
        assert np.max(np.abs(g_step[k])) > 0
        assert util.rel_err(g_mod[k], g_step[k]) < 1e-5, k
    # ... and the step-level path at n is the fresh context's
    f = model(util.SMALL, n, params)
    f.training()
    f.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    f.set_dropout_seed(77, 5)
    f.zero_grads()
    f.forward()
    f.backward(hop_w)
    for k, v in f.get_grads().items():
        assert np.array_equal(v, g_step[k]), k
    f.close()
    m.close()


# ---- 7. graph: keyed by the batch size
def test_graph_step_follows_the_batch_size():
    sh = util.shapes(util.MEDIUM)                 # capacity 70
    _, params, _ = util.make_problem(sh, scale=0.3)
    hop_w = np.full(sh.H, float(sh.H), np.float32)
    g, e = graph_model(sh, params), graph_model(sh, params)

    def step(m, batch, it, graph):
        m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
        m.set_dropout_seed(11, it)
        if graph:
            m.graph_step(hop_w)
        else:
            m.zero_grads()
            m.forward()
            m.backward(hop_w)
        gr = m.get_grads()
        return {"losses": m.losses(), "logits": m.logits(), **gr}
    full = np.full(sh.B, sh.T, np.int32)
    b70, _, _ = util.make_problem(sh, seed=50, lens=full, scale=0.3)
    b33, _, _ = util.make_problem(util.shapes(util.MEDIUM, B=33), seed=51, lens=full[:33], scale=0.3)
    before = step(g, b70, 0, True)
    same(before, step(e, b70, 0, False), "graph at capacity")
    same(step(g, b33, 1, True), step(e, b33, 1, False), "graph at 33 == eager at 33")     # set_batch resizes
    assert g.batch_size == 33 and g.logits().shape[1] == 33
    same(step(g, b70, 0, True), before, "graph back at capacity == before the excursion")
    g.close()
    e.close()


# ---- 8. errors and cleared state
def test_errors_and_cleared_state():
    n, cap = 5, 8
    batch, params, mc = problem(util.SMALL, cap)
    small, _, mc5 = problem(util.SMALL, n)
    m = model(util.SMALL, cap, params)
    lib, h = m._lib, m._h

    def size():
        a, b = L.C.c_int32(), L.C.c_int32()
        assert lib.rau_batch_size(h, L.C.byref(a), L.C.byref(b)) == 0
        return a.value, b.value
    for bad in (0, cap + 1, -3):
        assert lib.rau_set_batch_size(h, bad) == ERR_INVALID
        assert size() == (cap, cap)
    with pytest.raises(ValueError):
        m.set_batch_size(cap + 1)
    # a resize to the current size keeps the resident batch usable
    m.evaluate()
    m.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    assert lib.rau_set_batch_size(h, cap) == 0
    m.forward()
    m.predict(mc)
    # explicit masks and a slot upload made before the resize
    m.training()
    masks = util.make_problem(util.shapes(util.SMALL), scale=0.5)[2]
    m.set_masks(masks)
    m.set_batch_async(1, batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    m.set_batch_size(n)
    assert size() == (n, cap)
    assert lib.rau_forward(h) == ERR_STATE
    assert lib.rau_use_batch(h, 1) == ERR_STATE
    assert lib.rau_step_stats(h, None, None, None) == ERR_STATE
    assert lib.rau_predict(h, None, 0, None, None) == ERR_STATE
    assert lib.rau_get_merged(h, None, None) == ERR_STATE
    hw = np.ones(util.SMALL["H"], np.float32)
    assert lib.rau_backward(h, hw.ctypes.data) == ERR_STATE
    assert lib.rau_graph_step(h, hw.ctypes.data, 1) == ERR_STATE
    # seeded masks again, in the shapes of n
    m.set_dropout_seed(7, 3)
    f = model(util.SMALL, n, params)
    f.training()
    f.set_dropout_seed(7, 3)
    for site, shape in m.cfg.mask_shapes(n).items():
        got = m.get_mask(site)
        assert got.shape == shape and np.array_equal(got, f.get_mask(site)), site
        cut = masks[site][:, :n]
        assert not np.array_equal(got, cut)
    f.close()
    # rau_set_mask: the element count of n is accepted, that of the capacity rejected
    keep = np.ascontiguousarray(masks["q"][:, :n])
    assert lib.rau_set_mask(h, L.MASK_SITES["q"], keep.ctypes.data, keep.size) == 0
    full = np.ascontiguousarray(masks["q"])
    assert lib.rau_set_mask(h, L.MASK_SITES["q"], full.ctypes.data, full.size) == ERR_INVALID
    assert np.array_equal(m.get_mask("q"), keep)
    # python-side validation raises before any library call
    with pytest.raises(ValueError):
        m.set_batch(batch["feats"], batch["tokens"], np.zeros(cap + 1, np.int32), None)
    with pytest.raises(ValueError):
        m.set_batch(batch["feats"], batch["tokens"], small["lens"], None)          # 8 | 8 | 5 rows
    assert size() == (n, cap)
    # the inputs exist again: everything works at n
    m.evaluate()
    m.set_batch(small["feats"], small["tokens"], small["lens"], small["labels"])
    m.forward()
    oe, _ = m.predict(mc5)
    assert oe.shape == (util.SMALL["H"] + 2, n) and m.logits().shape == (util.SMALL["H"], n, util.SMALL["K"])
    m.close()
