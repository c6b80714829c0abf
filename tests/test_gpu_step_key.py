"""rau_graph_step's cache key (csrc: StepKey), walked member by member on ONE context.

The per-feature files each capture the two or three shapes of their own feature.  Here one context's cache is taken
from a base step to a step that differs from it in one key member and back, for every member; a twin context runs
the same steps eagerly (zero_grads; forward; backward).  After every step the losses, the logits and the three
gradient groups have the twin's bits.  A member left out of the key's equality replays the wrong graph at its
variant (or at the base step behind it) and fails here, while every per-feature file still passes.

Members that only change together with another one when they leave the base step (bank with table, att with
att_targets, the answer set's G between two sets) are also stepped between their two neighbours directly."""
import numpy as np
import pytest

from rau_vqa_amd import feat16
from tests import util
from tests.test_gpu_answers import answer_set

pytestmark = pytest.mark.gpu

D = util.SMALL
HOP_W = np.array([3.0, 1.0, 3.0], np.float32)


def _mk(params):
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**D))
    m.set_params(params)
    m.training()
    m.bank_create(6, "f32")
    return m


def _batch(sh, seed, max_len=None, rows=None):
    n = rows or sh.B
    lens = np.array([sh.T, 3, 5, 1, sh.T, 2, 4, 3], np.int32)[:n]      # ragged, longest = T
    if max_len:
        lens = np.minimum(lens, max_len)
    b = util.make_problem(util.shapes(D, B=n), seed=seed, lens=lens, scale=0.3)[0]
    return dict(feats=b["feats"], tokens=b["tokens"], lens=b["lens"], labels=b["labels"])


def test_every_key_member_selects_its_own_graph():
    sh = util.shapes(D)
    _, params, masks = util.make_problem(sh, scale=0.3)
    eager, graph = _mk(params), _mk(params)
    rng = np.random.default_rng(5)
    base, other = _batch(sh, 50), _batch(sh, 51)
    table = rng.standard_normal((6, sh.D, sh.S)).astype(np.float32)
    image_of = np.array([0, 5, 2, 2, 1, 4, 0, 3], np.int32)
    for m in (eager, graph):
        m.bank_put(0, table)
    no_feats = {k: v for k, v in base.items() if k != "feats"}
    tab = dict(no_feats, feats=table, image_of=image_of)
    bank = dict(no_feats, feats=None, bank_rows=np.arange(6, dtype=np.int32), image_of=image_of)
    targets = rng.random((sh.B, sh.S)).astype(np.float32)
    with_t = dict(base, att_targets=targets)
    att_w = np.array([0.5, 0.0, 2.0], np.float32)
    sets = {G: dict(base, answers=answer_set(D, G, seed=G)) for G in (2, 3)}

    def put(batch):
        return lambda m: m.set_batch(**batch)

    def slot1(m):
        m.set_batch_async(1, **other)
        m.use_batch(1)

    def slot0(m):
        m.set_batch_async(0, **base)
        m.use_batch(0)

    # name: (load the batch, hop_w, keyword arguments of the step); "leave" runs behind the step
    BASE = (put(base), HOP_W, {})
    variants = {
        "max_len": (put(_batch(sh, 50, max_len=4)), HOP_W, {}),
        "active": (put(base), np.array([3.0, 1.0, 0.0], np.float32), {}),
        "zero": (put(base), HOP_W, {"zero": False}),
        "mexplicit": (put(base), HOP_W, {"masks": {"q": masks["q"]}}),
        "B": (put(_batch(sh, 52, rows=5)), HOP_W, {}),
        "ans_G=2": (put(sets[2]), HOP_W, {}),
        "ans_G=3": (put(sets[3]), HOP_W, {}),
        "regions": (put(dict(base, regions=np.array([12, 1, 7, 12, 3, 9, 5, 11], np.int32))), HOP_W, {}),
        "att_targets": (put(with_t), HOP_W, {}),
        "sel": (put(base), HOP_W, {"select_w": np.array([0.5, 1.0, 0.25], np.float32)}),
        "att": (put(with_t), HOP_W, {"att_w": att_w}),
        "mrg": (put(base), HOP_W, {"merge_w": np.array([0.7, 1.3], np.float32)}),
        "feat_type": (put(dict(base, feats=feat16.bf16_bits(base["feats"]), feat_type="bf16")), HOP_W, {}),
        "slot": (slot1, HOP_W, {"leave": slot0}),
        "table": (put(tab), HOP_W, {}),
        "bank": (put(bank), HOP_W, {}),
        "mode": (put(base), HOP_W, {"mode": "evaluate"}),
    }
    walk = []
    for name in variants:
        walk += ["base", name]
    walk += ["base", "table", "bank", "table", "att_targets", "att", "att_targets", "ans_G=2", "ans_G=3", "ans_G=2",
             "base"]

    for it, name in enumerate(walk):
        load, hop_w, kw = BASE if name == "base" else variants[name]
        kw = dict(kw)
        zero, mode = kw.pop("zero", True), kw.pop("mode", "training")
        explicit, leave = kw.pop("masks", None), kw.pop("leave", None)
        outs = []
        for m in (eager, graph):
            getattr(m, mode)()
            load(m)
            m.set_dropout_seed(11, it)               # Philox masks at every site (and no explicit ones) ...
            if explicit:
                m.set_masks(explicit)                # ... but the caller's at this one
            if m is graph:
                m.graph_step(hop_w, zero_grads=zero, **kw)
            else:
                if zero:
                    m.zero_grads()
                m.forward()
                m.backward(hop_w, **kw)
            g = m.get_grads()
            outs.append((m.losses(), m.logits(), g["embed"], g["rnn"], g["mult"]))
            if leave:
                leave(m)
        for what, a, b in zip(("losses", "logits", "g_embed", "g_rnn", "g_mult"), *outs):
            assert a.shape == b.shape and np.array_equal(a, b), f"step {it} ({name}): {what}"
    eager.close()
    graph.close()
