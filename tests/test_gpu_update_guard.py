"""The non-finite guard in front of the three update calls (rau_set_update_guard), on util.SMALL in f32.

Bars: bit equality throughout.  A clean guarded step is an unguarded twin's step in every buffer, norm and count, with
the guard's two launches in front of the twin's; a poisoned step changes no bit anywhere, launches nothing of the
update, returns NaN norms and is counted; the update after it is the twin's.  No test here lets a NaN through an
unguarded update."""
import ctypes as C

import numpy as np
import pytest

from tests import util
from tests.test_gpu_update_ex import GROUPS, ex, new_model, opts, plain, same_bits, same_state, state

pytestmark = pytest.mark.gpu

INVALID = -1
GUARD_LAUNCHES = {"layer_stats_part": 1, "layer_stats_finish": 1}
# (call, rule, scope, extras): rau_noise_clip_adam is Adam with one clip per group
CLEAN = [("nca", "adam", "group", {})] + \
        [(call, rule, scope, {}) for call in ("update", "ex") for rule in ("adam", "adamax")
         for scope in ("group", "global")] + \
        [("ex", "adam", "global", dict(weight_decay=0.05, ema_decay=0.9))]
POISONED = [("nca", "adam", "group", {}), ("update", "adamax", "global", {}), ("ex", "adam", "group", {}),
            ("ex", "adamax", "global", dict(weight_decay=0.05, ema_decay=0.9))]


@pytest.fixture(scope="module")
def prob():
    """(parameters, three steps' finite gradients of 0.01 * randn: a clip of 0.1 engages); read-only."""
    _, params, _ = util.make_problem(util.shapes(util.SMALL))
    rng = np.random.default_rng(3)
    grads = [{k: (rng.standard_normal(v.size) * 0.01).astype(np.float32) for k, v in params.items()}
             for _ in range(3)]
    return params, grads


def nca(m, step_t, o):
    norms = np.full(3, -1.0, np.float32)
    rc = m._lib.rau_noise_clip_adam(m._h, step_t, o.lr, o.mult_lr, o.beta1, o.beta2, o.eps, o.eta, o.gamma, o.clip,
                                    o.noise_seed, norms.ctypes.data)
    return rc, norms


def step(m, call, step_t, rule, scope, extras):
    o = opts(rule, scope, eta=0.01, noise_seed=7)
    if call == "nca":
        return nca(m, step_t, o)
    if call == "update":
        return plain(m, step_t, o)
    return ex(m, step_t, o, **extras)


def pair(params, extras):
    """A guarded context and its unguarded twin."""
    g, t = new_model(util.SMALL, params), new_model(util.SMALL, params)
    if extras.get("ema_decay"):
        g.ema_reset()
        t.ema_reset()
    g.guard_updates()
    assert g.update_guard["mode"] == 1 and t.update_guard["mode"] == 0
    return g, t


def launches(m):
    out = {k: v["launches"] for k, v in m.prof().items() if v["launches"]}
    m.prof_reset()
    return out


@pytest.mark.parametrize("call,rule,scope,extras", CLEAN, ids=lambda v: str(v) if not isinstance(v, dict) else
                         ("extras" if v else "plain"))
def test_a_clean_guarded_step_is_the_unguarded_step(prob, call, rule, scope, extras):
    params, grads = prob
    g, t = pair(params, extras)
    for m in (g, t):
        m.reset_opt_state(rule)
        m.prof_enable(True)
        m.prof_reset()
    for k in range(2):
        g.set_grads(grads[k])
        t.set_grads(grads[k])
        (rcg, ng), (rct, nt) = step(g, call, k, rule, scope, extras), step(t, call, k, rule, scope, extras)
        assert rcg == 0 and rct == 0
        assert same_bits(ng, nt) and np.isfinite(ng).all(), (k, ng, nt)
        assert same_state(state(g), state(t)), k
        lg, lt = launches(g), launches(t)
        assert lt and not set(lt) & set(GUARD_LAUNCHES)
        assert lg == {**lt, **GUARD_LAUNCHES}, (lg, lt)        # the twin's launches, the guard's two in front
        assert g.update_guard == {"mode": 1, "skipped": 0, "last_skipped": False,
                                  "last_nonfinite": {k_: 0 for k_ in GROUPS}}
    assert state(g)[1] == {k_: 2 for k_ in GROUPS}
    for m in (g, t):
        m.prof_enable(False)
        m.close()


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("call,rule,scope,extras", POISONED, ids=lambda v: str(v) if not isinstance(v, dict) else
                         ("extras" if v else "plain"))
def test_a_poisoned_step_is_skipped_and_leaves_no_trace(prob, call, rule, scope, extras, value):
    params, grads = prob
    g, t = pair(params, extras)
    for m in (g, t):
        m.reset_opt_state(rule)
    g.prof_enable(True)
    n_norms = 3 if call == "nca" else 4
    skipped = 0
    for k in range(2):          # before the first update (no moments yet, t = 0) and after one
        for gi, group in enumerate(GROUPS):
            bad = {name: v.copy() for name, v in grads[2].items()}
            at = (7 * (gi + 1) + k) % bad[group].size
            bad[group][at] = value
            g.set_grads(bad)
            before = state(g)
            g.prof_reset()
            rc, norms = step(g, call, k, rule, scope, extras)
            assert rc == 0
            assert norms.shape == (n_norms,) and np.isnan(norms).all(), norms
            assert same_state(before, state(g)), (k, group)          # x, g, m, v, the average, t and the rule
            assert launches(g) == GUARD_LAUNCHES                      # nothing of the update: no upd_*, no clip_adam
            skipped += 1
            want = {name: (1 if name == group else 0) for name in GROUPS}
            assert g.update_guard == {"mode": 1, "skipped": skipped, "last_skipped": True, "last_nonfinite": want}
        # a finite gradient again: the next update is the twin's, bit for bit
        g.set_grads(grads[k])
        t.set_grads(grads[k])
        (rcg, ng), (rct, nt) = step(g, call, k, rule, scope, extras), step(t, call, k, rule, scope, extras)
        assert rcg == 0 and rct == 0 and same_bits(ng, nt)
        assert same_state(state(g), state(t)), k
        assert g.update_guard["last_skipped"] is False and g.update_guard["skipped"] == skipped
    assert t.update_guard["skipped"] == 0
    g.prof_enable(False)
    g.close()
    t.close()


def test_the_python_update_returns_nan_norms_when_skipped(prob):
    params, grads = prob
    m = new_model(util.SMALL, params)
    m.guard_updates()
    bad = {name: v.copy() for name, v in grads[0].items()}
    bad["rnn"][-1] = -np.inf
    m.set_grads(bad)
    x0 = m.get_params()
    for kw, n in ((dict(), 3), (dict(rule="adamax"), 4), (dict(weight_decay=0.1), 4)):
        norms = m.update(0, **kw)
        assert norms.shape == (n,) and np.isnan(norms).all()
    assert m.update_guard["skipped"] == 3 and m.update_guard["last_nonfinite"] == {"embed": 0, "rnn": 1, "mult": 0}
    assert all(same_bits(x0[k], v) for k, v in m.get_params().items())
    assert m.opt_state()[0]["rnn"][2] == 0
    m.zero_grads()                       # what clears an accumulated NaN
    assert np.isfinite(m.update(0)).all() and m.update_guard["last_skipped"] is False
    m.close()


def test_a_frozen_layers_nan_skips_rau_update_but_not_rau_update_ex(prob):
    params, grads = prob
    g, t = pair(params, {})
    name = "classifier.out_score"
    for m in (g, t):
        assert m.freeze(name) == [name]
    lay = {e[0]: e for e in g.layout("mult")}
    a = lay[name + ".weight"][1]
    b = lay[name + ".bias"][1] + lay[name + ".bias"][2]
    bad = {k: v.copy() for k, v in grads[0].items()}
    bad["mult"][a], bad["mult"][b - 1] = np.nan, np.inf      # the layer's first weight and its last bias element
    for m in (g, t):
        m.set_grads(bad)                 # the twin never reads a frozen element either: nothing bad is let through
    before = state(g)
    o = opts("adam", "global", eta=0.01, noise_seed=7)
    (rcg, ng), (rct, nt) = ex(g, 0, o), ex(t, 0, o)
    assert rcg == 0 and rct == 0 and np.isfinite(ng).all() and same_bits(ng, nt)
    assert g.update_guard["last_skipped"] is False and g.update_guard["skipped"] == 0
    after = state(g)
    assert same_state(after, state(t))
    for buf in ("x", "g", "m", "v"):     # the frozen layer keeps its bits, the NaN in its gradient included
        assert same_bits(before[0][buf]["mult"][a:b], after[0][buf]["mult"][a:b]), buf
    assert not same_bits(before[0]["x"]["mult"][:a], after[0]["x"]["mult"][:a])
    # rau_update does not look at layer options: the same NaN skips it
    rc, norms = plain(g, 1, o)
    assert rc == 0 and np.isnan(norms).all() and same_state(after, state(g))
    assert g.update_guard["skipped"] == 1 and g.update_guard["last_nonfinite"] == {"embed": 0, "rnn": 0, "mult": 2}
    g.close()
    t.close()


def test_the_guard_outlives_set_batch_size_and_switches_off_again(prob):
    params, grads = prob
    m = new_model(util.SMALL, params)
    lib = m._lib
    assert m.update_guard == {"mode": 0, "skipped": 0, "last_skipped": False,
                              "last_nonfinite": {k: 0 for k in GROUPS}}
    m.guard_updates()
    for mode in (2, -1, 7):
        assert lib.rau_set_update_guard(m._h, mode) == INVALID
    assert m.update_guard["mode"] == 1
    m.set_batch_size(4)
    assert m.update_guard["mode"] == 1 and m.batch_size == 4
    o = opts("adam", "group", eta=0.01, noise_seed=7)
    m.set_grads(grads[0])
    m.prof_enable(True)
    m.prof_reset()
    assert plain(m, 0, o)[0] == 0
    assert launches(m) == {"upd_noise_sqnorm": 1, "upd_apply": 1, **GUARD_LAUNCHES}
    m.guard_updates(False)
    assert m.update_guard["mode"] == 0
    m.set_grads(grads[1])
    assert plain(m, 1, o)[0] == 0
    assert launches(m) == {"upd_noise_sqnorm": 1, "upd_apply": 1}      # today's launch list
    assert lib.rau_update_guard(m._h, None, None, None, None) == 0      # every output may be NULL
    m.prof_enable(False)
    m.close()
