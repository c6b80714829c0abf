"""rau_update_ex's host side: the fp64 statement (tests/update_ex_ref.py) pinned to torch.optim.AdamW, the frozen
exclusion, the header and its ctypes mirror, which library call RAU.update makes, layer names, the snapshot field."""
import os
import re

import numpy as np
import pytest

from tests import update_ex_ref, update_ref
from tests.update_ex_ref import Seg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = update_ref.GROUPS


def test_adam_with_decay_is_torch_adamw_at_eps_0():
    """Five steps in fp64.  eps = 0: the project keeps eps outside the bias-corrected sqrt, torch inside its own
    form, so the two agree only there."""
    import torch
    rng = np.random.default_rng(5)
    n, lr, b1, b2, wd = 257, 2e-3, 0.9, 0.999, 0.05
    x0 = rng.standard_normal(n)
    p = torch.tensor(x0.copy(), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=0.0, weight_decay=wd)
    sizes = {"embed": n, "rnn": 3, "mult": 3}
    segs = {k: [Seg(s)] for k, s in sizes.items()}
    x = {k: (x0.copy() if k == "embed" else np.ones(s)) for k, s in sizes.items()}
    m = {k: np.zeros(s) for k, s in sizes.items()}
    v = {k: np.zeros(s) for k, s in sizes.items()}
    worst = 0.0
    for t in range(1, 6):
        g = {k: rng.standard_normal(s) * 0.01 for k, s in sizes.items()}
        p.grad = torch.tensor(g["embed"].copy(), dtype=torch.float64)
        opt.step()
        x, _, m, v, _, _ = update_ex_ref.update(x, g, m, v, None, {k: t for k in sizes}, t - 1, segs, lr=lr, b1=b1,
                                                b2=b2, eps=0.0, eta=0.0, clip=1e30, weight_decay=wd)
        worst = max(worst, float(np.max(np.abs(x["embed"] - p.detach().numpy()))))
    print(f"max |statement - AdamW| over five steps: {worst:.2e}")
    assert worst < 1e-12
    assert np.max(np.abs(m["embed"] - opt.state[p]["exp_avg"].numpy())) < 1e-12
    assert np.max(np.abs(v["embed"] - opt.state[p]["exp_avg_sq"].numpy())) < 1e-12


def _problem(rng, sizes):
    x = {k: rng.standard_normal(n) for k, n in sizes.items()}
    g = {k: rng.standard_normal(n) for k, n in sizes.items()}
    z = {k: np.zeros(n) for k, n in sizes.items()}
    return x, g, z


def test_defaults_are_the_old_statement():
    rng = np.random.default_rng(1)
    sizes = {"embed": 21, "rnn": 30, "mult": 45}
    segs = {"embed": [Seg(21)], "rnn": [Seg(13), Seg(30, decay=0.0)], "mult": [Seg(5), Seg(6, decay=0.0), Seg(45)]}
    x, g, z = _problem(rng, sizes)
    noise = {k: rng.standard_normal(n) for k, n in sizes.items()}
    for rule in ("adam", "adamax"):
        for scope in ("group", "global"):
            a = update_ref.update(x, g, z, z, {k: 1 for k in sizes}, 3, noise=noise, rule=rule, clip_scope=scope)
            b = update_ex_ref.update(x, g, z, z, None, {k: 1 for k in sizes}, 3, segs, noise=noise, rule=rule,
                                     clip_scope=scope)
            for k in sizes:
                for i, j in ((0, 0), (1, 1), (2, 2), (3, 3)):
                    assert np.array_equal(a[i][k], b[j][k]), (rule, scope, k, i)
            assert np.array_equal(a[4], b[5])


def test_frozen_segments_are_in_no_norm_and_keep_everything():
    rng = np.random.default_rng(2)
    sizes = {"embed": 12, "rnn": 30, "mult": 45}
    segs = {"embed": [Seg(12, lr_scale=0.0)],                      # a whole group frozen
            "rnn": [Seg(13), Seg(30)],
            "mult": [Seg(5), Seg(6, lr_scale=0.0), Seg(41, lr_scale=0.0), Seg(45)]}
    x, g, z = _problem(rng, sizes)
    e = {k: rng.standard_normal(n) for k, n in sizes.items()}
    noise = {k: rng.standard_normal(n) for k, n in sizes.items()}
    xo, go, mo, vo, eo, norms = update_ex_ref.update(x, g, z, z, e, {k: 1 for k in sizes}, 0, segs, noise=noise,
                                                     clip_scope="global", weight_decay=0.1, ema_decay=0.9)
    nstd = np.sqrt(0.01 / 0.55)
    live = {"embed": np.zeros(12, bool), "rnn": np.ones(30, bool),
            "mult": np.r_[np.ones(5, bool), np.zeros(36, bool), np.ones(4, bool)]}
    want = [np.sqrt(np.sum((g[k] + noise[k] * nstd)[live[k]] ** 2)) for k in GROUPS]
    assert norms[0] == 0.0
    assert np.allclose(norms[:3], want, rtol=1e-14)
    assert abs(norms[3] - np.sqrt(want[1] ** 2 + want[2] ** 2)) < 1e-13
    for k in GROUPS:
        f = ~live[k]
        for new, old in ((xo, x), (go, g), (mo, z), (vo, z), (eo, e)):
            assert np.array_equal(new[k][f], old[k][f]), k                    # frozen: every value kept, no noise
            assert not np.any(new[k][live[k]] == old[k][live[k]]), k          # the rest moved
    # the clip is the live elements' global norm
    assert np.allclose(go["rnn"], (g["rnn"] + noise["rnn"] * nstd) * (0.1 / norms[3]), rtol=1e-14)


def test_decay_comes_before_the_step_and_the_average_after():
    sizes = {"embed": 2, "rnn": 2, "mult": 2}
    segs = {"embed": [Seg(2, lr_scale=0.5)], "rnn": [Seg(1), Seg(2, decay=0.0)], "mult": [Seg(2)]}
    x = {k: np.array([2.0, -3.0]) for k in sizes}
    g = {k: np.array([0.01, -0.02]) for k in sizes}
    z = {k: np.zeros(2) for k in sizes}
    e = {k: np.array([1.0, 1.0]) for k in sizes}
    xo, go, mo, vo, eo, _ = update_ex_ref.update(x, g, z, z, e, {k: 1 for k in sizes}, 0, segs, lr=0.1, mult_lr=0.01,
                                                 eps=0.0, eta=0.0, clip=1e30, weight_decay=0.5, ema_decay=0.75)
    # t = 1, eps = 0: Adam's step is lr * sign(g)
    assert np.allclose(xo["embed"], x["embed"] * (1 - 0.1 * 0.5 * 0.5) - 0.05 * np.sign(g["embed"]), rtol=1e-15)
    assert np.allclose(xo["rnn"], x["rnn"] * np.array([1 - 0.1 * 0.5, 1.0]) - 0.1 * np.sign(g["rnn"]), rtol=1e-15)
    assert np.allclose(xo["mult"], x["mult"] * (1 - 0.01 * 0.5) - 0.01 * np.sign(g["mult"]), rtol=1e-15)
    for k in sizes:
        assert np.allclose(eo[k], 0.75 * e[k] + 0.25 * xo[k], rtol=1e-15)
        assert np.array_equal(go[k], g[k]) and np.allclose(mo[k], 0.1 * g[k], rtol=1e-12)   # decay: not in g, m


def test_header_declares_the_calls_and_the_mirror_follows_it():
    text = open(os.path.join(ROOT, "include", "rau.h")).read()
    assert re.search(r"#define\s+RAU_ABI_VERSION\s+5\b", text)
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn in ("rau_update_extras_default", "rau_update_ex", "rau_set_layer_opts", "rau_get_layer_opts",
               "rau_ema_reset", "rau_ema_swap", "rau_ema_state", "rau_get_ema", "rau_set_ema"):
        assert re.search(r"\b%s\s*\(" % fn, code), fn
    from rau_vqa_amd import _lib
    assert all(fn in _lib._SIGS for fn in ("rau_update_ex", "rau_set_layer_opts", "rau_ema_swap"))
    body = re.search(r"typedef struct rau_update_extras \{(.*?)\} rau_update_extras;", code, flags=re.S).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip()
              for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == ["weight_decay", "ema_decay"]
    assert [n for n, _ in _lib.RauUpdateExtras._fields_] == fields
    # rau_update_opts is what it was
    body = re.search(r"typedef struct rau_update_opts \{(.*?)\}", code, flags=re.S).group(1)
    assert "weight_decay" not in body and "ema" not in body
    # the contract names its roundings and the Adamax form
    for phrase in ("AdamW", "NOT torch.optim.Adamax's L2 term", "both products and the sum rounded", "frozen"):
        assert phrase in text, phrase
    # the Lua cdef carries the same struct
    lua = open(os.path.join(ROOT, "bindings", "rau.lua")).read()
    assert re.search(r"typedef struct rau_update_extras \{\s*float weight_decay;\s*float ema_decay;\s*\} "
                     r"rau_update_extras;", lua)
    for fn in ("updateEx", "setLayerOpts", "emaReset", "emaSwap"):
        assert re.search(r"function RAU:%s\b" % fn, lua), fn


class _FakeLib:
    """Records the library calls; every call succeeds; layer options read back as their defaults."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rau_get_layer_opts":
                for ref, val in zip(args[3:], (1.0, 1.0, 0.0)):
                    ref._obj.value = val
            return 0
        return fn


LAYOUTS = {"embed": [("word_embed.weight", 0, 9, 4)],
           "rnn": [("rnn.l1.i2h.weight", 0, 16, 4), ("rnn.l1.i2h.bias", 64, 16, 1),
                   ("rnn.l1.h2h.weight", 80, 16, 4), ("rnn.l1.h2h.bias", 144, 16, 1)],
           "mult": [("attbycontent.attscore.weight", 0, 1, 4), ("attbycontent.attscore.bias", 4, 1, 1),
                    ("classifier.lstm_out.weight", 5, 4, 4), ("classifier.lstm_out.bias", 21, 4, 1),
                    ("classifier.out_score.weight", 25, 4, 4), ("classifier.out_score.bias", 41, 4, 1)]}


def _fake_rau():
    from rau_vqa_amd import model
    m = object.__new__(model.RAU)
    m._lib, m._h = _FakeLib(), None
    m._layers = model.layer_units(LAYOUTS)
    return m


def _names(m):
    return [c[0] for c in m._lib.calls if c[0] != "rau_get_layer_opts"]


def test_update_routes_to_update_ex_only_for_the_new_arguments():
    from rau_vqa_amd import _lib as L
    m = _fake_rau()
    assert _names(m) == [] and m.update(step_t=4, lr=1e-3).shape == (3,)
    assert _names(m) == ["rau_noise_clip_adam"]                     # old arguments: the old calls
    m._lib.calls.clear()
    assert m.update(step_t=4, rule="adamax", weight_decay=0.0, ema_decay=0.0).shape == (4,)
    assert _names(m) == ["rau_update"]
    for kw in (dict(weight_decay=0.01), dict(ema_decay=0.999), dict(weight_decay=0.01, rule="adamax"),
               dict(ema_decay=0.5, clip_scope="global")):
        m._lib.calls.clear()
        norms = m.update(step_t=2, lr=2e-3, noise_seed=5, **kw)
        assert _names(m) == ["rau_update_ex"] and norms.shape == (4,)
        _, step_t, o, x, _ = m._lib.calls[0][1]
        assert step_t == 2 and o._obj.noise_seed == 5 and abs(o._obj.lr - 2e-3) < 1e-9
        assert o._obj.rule == L.OPT_RULES[kw.get("rule", "adam")]
        assert o._obj.clip_scope == L.CLIP_SCOPES[kw.get("clip_scope", "group")]
        assert x._obj.weight_decay == np.float32(kw.get("weight_decay", 0.0))
        assert x._obj.ema_decay == np.float32(kw.get("ema_decay", 0.0))
    # a layer option off its default routes every update there, until it is back at the default
    m._lib.calls.clear()
    assert m.freeze("classifier.lstm_out") == ["classifier.lstm_out"]
    assert ("rau_set_layer_opts", (None, 2, 1, 0.0, 1.0, 0.0)) in m._lib.calls
    m._lib.calls.clear()
    m.update(step_t=0)
    assert _names(m) == ["rau_update_ex"]
    m.unfreeze("classifier.lstm_out")
    m._lib.calls.clear()
    m.update(step_t=0)
    assert _names(m) == ["rau_noise_clip_adam"]
    for kw in (dict(rule="sgd"), dict(clip_scope="layer")):
        m._lib.calls.clear()
        with pytest.raises(ValueError):
            m.update(step_t=0, weight_decay=0.1, **kw)
        assert not m._lib.calls


def test_layer_names_and_globs_resolve_against_the_layout():
    from rau_vqa_amd.model import layer_units, match_layers
    units = layer_units(LAYOUTS)
    assert units == [("word_embed", "embed", 0), ("rnn.l1.i2h", "rnn", 0), ("rnn.l1.h2h", "rnn", 1),
                     ("attbycontent.attscore", "mult", 0), ("classifier.lstm_out", "mult", 1),
                     ("classifier.out_score", "mult", 2)]
    assert match_layers("classifier.out_score", units) == [("classifier.out_score", "mult", 2)]
    assert match_layers("word_embed.weight", units) == [("word_embed", "embed", 0)]       # an entry's own name
    assert match_layers("rnn.l1.h2h.bias", units) == [("rnn.l1.h2h", "rnn", 1)]
    assert [u[0] for u in match_layers("classifier.*", units)] == ["classifier.lstm_out", "classifier.out_score"]
    assert [u[0] for u in match_layers("rnn.l1.?2h", units)] == ["rnn.l1.i2h", "rnn.l1.h2h"]
    assert len(match_layers("*", units)) == 6
    for bad in ("classifier", "out_score", "rnn.l2.*", ""):
        with pytest.raises(KeyError):
            match_layers(bad, units)
    with pytest.raises(ValueError):
        layer_units(dict(LAYOUTS, rnn=LAYOUTS["rnn"][1:]))
    # set_layer_opts keeps what is None and passes group and unit index
    m = _fake_rau()
    assert m.set_layer_opts("rnn.*", lr_scale=0.25, bias_decay=1.0) == ["rnn.l1.i2h", "rnn.l1.h2h"]
    sets = [c[1][1:] for c in m._lib.calls if c[0] == "rau_set_layer_opts"]
    assert sets == [(1, 0, 0.25, 1.0, 1.0), (1, 1, 0.25, 1.0, 1.0)]


def test_snapshot_ema_field_round_trips_and_its_absence_changes_nothing(tmp_path):
    from rau_vqa_amd import t7
    rng = np.random.default_rng(0)
    sizes = {"embed": 11, "rnn": 7, "mult": 13}
    params = {k: rng.standard_normal(n).astype(np.float32) for k, n in sizes.items()}
    ema = {k: rng.standard_normal(n).astype(np.float32) for k, n in sizes.items()}
    state = {k: (np.zeros(n, np.float32), np.ones(n, np.float32), 2) for k, n in sizes.items()}
    plain, none, full = (str(tmp_path / f) for f in ("plain.t7", "none.t7", "full.t7"))
    t7.save_snapshot(plain, params, 120, 3, {"lr": 3e-3}, optim=(state, "adam"))
    t7.save_snapshot(none, params, 120, 3, {"lr": 3e-3}, optim=(state, "adam"), ema=None)
    t7.save_snapshot(full, params, 120, 3, {"lr": 3e-3}, optim=(state, "adam"), ema=ema)
    assert open(plain, "rb").read() == open(none, "rb").read()            # without it: the file of before
    assert t7.load_ema(plain) is None and "ema" not in t7.load(plain)
    it, epoch, opt, got = t7.load_snapshot(full)                          # the old readers' results are unchanged
    assert (it, epoch, opt) == (120, 3, {"lr": 3e-3})
    assert all(np.array_equal(got[k], params[k]) for k in params)
    assert t7.load_optim(full)[1] == "adam"
    back = t7.load_ema(full)
    assert all(np.array_equal(back[k], ema[k]) and back[k].dtype == np.float32 for k in sizes)
    snap = t7.load(full)
    assert sorted(snap) == ["ema", "epoch", "it", "opt", "optim", "params"]
    with pytest.raises(t7.T7Error):
        t7.load_ema(dict(snap, ema={1: snap["ema"][1]}))
    # RAU.load_snapshot hands it to rau_set_ema; one without the field leaves the average alone
    m = _fake_rau()
    m.group_size = lambda g: sizes[g]
    m.load_snapshot(plain)
    assert "rau_set_ema" not in _names(m)
    m._lib.calls.clear()
    m.load_snapshot(full)
    assert _names(m).count("rau_set_ema") == 3
