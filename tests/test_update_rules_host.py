"""rau_update's host side: the fp64 statement pinned to torch's Adamax and to the reference update's
restatement, the header, the snapshot field, and which library call RAU.update makes."""
import os
import re

import numpy as np
import pytest

from tests import update_ref
from tests.test_update import adam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numpy_adamax_is_torch_adamax():
    """Five steps, some gradient entries exactly 0 (u = max(b2 u, eps) there, a finite step of 0 at t = 1)."""
    import torch
    rng = np.random.default_rng(5)
    n, lr, b1, b2, eps = 257, 2e-3, 0.9, 0.999, 1e-8
    x0 = rng.standard_normal(n)
    p = torch.tensor(x0.copy(), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adamax([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=0)
    x, m, u = x0.copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * 0.01
        g[::7] = 0.0
        if t == 1:
            g[:5] = 0.0
        p.grad = torch.tensor(g.copy(), dtype=torch.float64)
        opt.step()
        x, m, u = update_ref.adamax_elem(x, g, m, u, t, lr, b1, b2, eps)
        assert np.all(np.isfinite(x))
        assert np.max(np.abs(x - p.detach().numpy())) < 1e-12
        if t == 1:
            assert np.array_equal(x[:5], x0[:5]) and np.all(u[:5] == eps)   # u = eps, a step of exactly 0
    st = opt.state[p]
    assert np.max(np.abs(m - st["exp_avg"].numpy())) < 1e-12
    assert np.max(np.abs(u - st["exp_inf"].numpy())) < 1e-12


def test_group_clip_adam_statement_is_the_old_statement():
    """rule = adam, clip_scope = group: tests/test_update.py's adam_ref per group, noise included."""
    rng = np.random.default_rng(11)
    sizes = {"embed": 301, "rnn": 57, "mult": 1000}
    x = {k: rng.standard_normal(n) for k, n in sizes.items()}
    m = {k: np.zeros(n) for k, n in sizes.items()}
    v = {k: np.zeros(n) for k, n in sizes.items()}
    xr, mr, vr = ({k: a.copy() for k, a in d.items()} for d in (x, m, v))
    for t in range(1, 4):
        g = {k: rng.standard_normal(n) * 0.01 for k, n in sizes.items()}
        noise = {k: rng.standard_normal(n) for k, n in sizes.items()}
        x, gc, m, v, norms = update_ref.update(x, g, m, v, {k: t for k in sizes}, t - 1, noise=noise)
        for i, k in enumerate(update_ref.GROUPS):
            lr = 3e-4 if k == "mult" else 3e-3
            xr[k], g2, mr[k], vr[k], n_ref = adam_ref(xr[k], g[k], mr[k], vr[k], noise[k], t - 1, t, lr)
            assert abs(norms[i] - n_ref) < 1e-14
            for a, b in ((x[k], xr[k]), (gc[k], g2), (m[k], mr[k]), (v[k], vr[k])):
                assert np.allclose(a, b, rtol=1e-13, atol=1e-16), k
        assert abs(norms[3] - np.sqrt(sum(norms[i] ** 2 for i in range(3)))) < 1e-14


def test_global_clip_uses_one_scale():
    rng = np.random.default_rng(2)
    sizes = {"embed": 40, "rnn": 30, "mult": 50}
    z = {k: np.zeros(n) for k, n in sizes.items()}
    g = {k: rng.standard_normal(n) for k, n in sizes.items()}
    _, gc, _, _, norms = update_ref.update(z, g, z, z, {k: 1 for k in sizes}, 0, rule="adamax",
                                           clip_scope="global", clip=0.1)
    assert norms[3] > 0.1
    for k in sizes:
        assert np.allclose(gc[k], g[k] * (0.1 / norms[3]), rtol=1e-15)
    total = np.sqrt(sum(np.sum(gc[k] ** 2) for k in sizes))
    assert abs(total - 0.1) < 1e-12


def test_header_declares_the_update_calls():
    text = open(os.path.join(ROOT, "include", "rau.h")).read()
    assert re.search(r"#define\s+RAU_ABI_VERSION\s+5\b", text)
    for name, value in (("RAU_OPT_ADAM", 0), ("RAU_OPT_ADAMAX", 1), ("RAU_CLIP_GROUP", 0), ("RAU_CLIP_GLOBAL", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn in ("rau_update_opts_default", "rau_update", "rau_get_opt_state", "rau_set_opt_state",
               "rau_dev_adamax", "rau_noise_clip_adam"):
        assert re.search(r"\b%s\s*\(" % fn, code), fn
    assert re.search(r"typedef struct rau_update_opts \{.*?\} rau_update_opts;", code, flags=re.S)
    assert "SS:597-630" in text and "NOT in the reference" in text
    # the ctypes mirror of the struct has the header's fields in the header's order
    from rau_vqa_amd import _lib
    body = re.search(r"typedef struct rau_update_opts \{(.*?)\}", code, flags=re.S).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip()
              for n in decl.strip().split(None, 1)[1].split(",")]
    assert [n for n, _ in _lib.RauUpdateOpts._fields_] == fields


def test_snapshot_optim_field_round_trips(tmp_path):
    from rau_vqa_amd import t7
    rng = np.random.default_rng(0)
    sizes = {"embed": 11, "rnn": 7, "mult": 13}
    params = {k: rng.standard_normal(n).astype(np.float32) for k, n in sizes.items()}
    state = {k: (rng.standard_normal(n).astype(np.float32), np.abs(rng.standard_normal(n)).astype(np.float32), 4 + i)
             for i, (k, n) in enumerate(sizes.items())}
    plain, full = str(tmp_path / "plain.t7"), str(tmp_path / "full.t7")
    t7.save_snapshot(plain, params, 120, 3, {"lr": 3e-3})
    t7.save_snapshot(full, params, 120, 3, {"lr": 3e-3}, optim=(state, "adamax"))
    # without the field: as before, and the separate reader says so
    it, epoch, opt, got = t7.load_snapshot(plain)
    assert (it, epoch, opt) == (120, 3, {"lr": 3e-3})
    assert all(np.array_equal(got[k], params[k]) for k in params)
    assert t7.load_optim(plain) is None
    assert "optim" not in t7.load(plain)
    # with it: the old reader's return value is unchanged, the field comes back bit for bit
    it, epoch, opt, got = t7.load_snapshot(full)
    assert (it, epoch, opt) == (120, 3, {"lr": 3e-3})
    assert all(np.array_equal(got[k], params[k]) for k in params)
    st, rule = t7.load_optim(full)
    assert rule == "adamax"
    for k in sizes:
        assert np.array_equal(st[k][0], state[k][0]) and np.array_equal(st[k][1], state[k][1])
        assert st[k][2] == state[k][2] and st[k][0].dtype == np.float32
    snap = t7.load(full)
    assert sorted(snap) == ["epoch", "it", "opt", "optim", "params"]       # one field beside params
    assert t7.load_optim(snap)[1] == "adamax"
    bad = dict(snap, optim={"rule": "adamax", "state": {1: {"m": 1}}})
    with pytest.raises(t7.T7Error):
        t7.load_optim(bad)


class _FakeLib:
    """Records which update entry point is called; every call succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _fake_rau():
    from rau_vqa_amd.model import RAU
    m = object.__new__(RAU)
    m._lib, m._h = _FakeLib(), None
    return m


def test_update_routes_by_rule_and_scope():
    from rau_vqa_amd import _lib as L
    m = _fake_rau()
    norms = m.update(step_t=4, lr=1e-3, noise_seed=9)
    assert [c[0] for c in m._lib.calls] == ["rau_noise_clip_adam"] and norms.shape == (3,)
    args = m._lib.calls[0][1]
    assert args[1] == 4 and args[2] == 1e-3 and args[10] == 9           # the old call, argument for argument
    for kw, rule, scope in ((dict(rule="adamax"), L.OPT_ADAMAX, L.CLIP_GROUP),
                            (dict(clip_scope="global"), L.OPT_ADAM, L.CLIP_GLOBAL),
                            (dict(rule="adamax", clip_scope="global"), L.OPT_ADAMAX, L.CLIP_GLOBAL)):
        m._lib.calls.clear()
        norms = m.update(step_t=2, lr=2e-3, clip=0.25, noise_seed=5, **kw)
        assert [c[0] for c in m._lib.calls] == ["rau_update"] and norms.shape == (4,)
        _, step_t, ref, _ = m._lib.calls[0][1]
        o = ref._obj
        assert step_t == 2 and (o.rule, o.clip_scope, o.noise_seed) == (rule, scope, 5)
        assert abs(o.lr - 2e-3) < 1e-9 and abs(o.clip - 0.25) < 1e-9 and abs(o.mult_lr - 3e-4) < 1e-9
    for kw in (dict(rule="sgd"), dict(clip_scope="layer")):
        m._lib.calls.clear()
        with pytest.raises(ValueError):
            m.update(step_t=0, **kw)
        assert not m._lib.calls


def test_reset_opt_state_passes_null_vectors():
    from rau_vqa_amd import _lib as L
    m = _fake_rau()
    m.reset_opt_state(rule="adamax")
    assert [(c[0], c[1][1:]) for c in m._lib.calls] == \
        [("rau_set_opt_state", (g, None, None, 0, L.OPT_ADAMAX)) for g in (0, 1, 2)]
