"""rau_update_ex on the device: decoupled weight decay, per-layer step sizes, frozen layers, the weight average.

Bars: bit equality wherever two device paths state the same arithmetic (defaults against rau_update, power-of-two
scales against halved step sizes, frozen layers against zeroed gradients); against the fp64 statement
(tests/update_ex_ref.py) the bar tests/test_gpu_update_rules.py holds rau_update to: util.rel_err < 1e-5 on weights,
moments and the average, 1e-5 * max(1, n) on norms.

Shapes: util.SMALL (the MULT offsets behind attscore are odd) and util.EDGE, the smallest layout at which the
segment cursor can go wrong: every width is 4, attscore is 4 + 1 floats, out_do_pred has a 1-float bias, and one
quad spans several segments."""
import ctypes as C

import numpy as np
import pytest

from tests import update_ex_ref, update_ref, util
from tests.test_update import device_normals

pytestmark = pytest.mark.gpu

GROUPS = update_ref.GROUPS
KEYS = ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")
BIG = dict(B=4, T=4, V=6000, E=200, Rq=64, D=64, S=196, M=512, A=256, R=512, K=1000, H=2)
DIMS = {"small": util.SMALL, "edge": util.EDGE}
INVALID, STATE = -1, -3
RULE_SCOPE = [("adam", "group"), ("adam", "global"), ("adamax", "group"), ("adamax", "global")]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def new_model(dims, params=None):
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**{k: dims[k] for k in KEYS}))
    if params is None:
        m.init_uniform(seed=1)
    else:
        m.set_params(params)
    return m


@pytest.fixture(scope="module", params=sorted(DIMS))
def prob(request):
    """(dims, parameters, three steps' gradients of 0.01 * randn: a clip of 0.1 engages at SMALL); read-only."""
    dims = DIMS[request.param]
    _, params, _ = util.make_problem(util.shapes(dims))
    rng = np.random.default_rng(3)
    grads = [{k: (rng.standard_normal(v.size) * 0.01).astype(np.float32) for k, v in params.items()}
             for _ in range(3)]
    return dims, params, grads


@pytest.fixture(scope="module")
def small():
    _, params, _ = util.make_problem(util.shapes(util.SMALL))
    rng = np.random.default_rng(3)
    grads = [{k: (rng.standard_normal(v.size) * 0.01).astype(np.float32) for k, v in params.items()}
             for _ in range(3)]
    return util.SMALL, params, grads


def opts(rule="adam", scope="group", **kw):
    from rau_vqa_amd import _lib as L
    o = L.RauUpdateOpts()
    L.lib().rau_update_opts_default(C.byref(o))
    o.rule, o.clip_scope = L.OPT_RULES[rule], L.CLIP_SCOPES[scope]
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def plain(m, step_t, o):
    norms = np.full(4, -1.0, np.float32)
    return m._lib.rau_update(m._h, step_t, C.byref(o), norms.ctypes.data), norms


def ex(m, step_t, o, weight_decay=0.0, ema_decay=0.0, null_extras=False):
    from rau_vqa_amd import _lib as L
    x = L.RauUpdateExtras(weight_decay=weight_decay, ema_decay=ema_decay)
    norms = np.full(4, -1.0, np.float32)
    rc = m._lib.rau_update_ex(m._h, step_t, C.byref(o), None if null_extras else C.byref(x), norms.ctypes.data)
    return rc, norms


def state(m):
    """Every buffer an update reads or writes, as one {name: {group: array}} plus the counts and the rule."""
    st, rule = m.opt_state()
    out = {"x": m.get_params(), "g": m.get_grads(), "m": {k: st[k][0] for k in GROUPS},
           "v": {k: st[k][1] for k in GROUPS}}
    if m.has_ema:
        out["e"] = m.ema()
    return out, {k: st[k][2] for k in GROUPS}, rule


def same_state(a, b):
    return a[1:] == b[1:] and sorted(a[0]) == sorted(b[0]) and \
        all(same_bits(a[0][n][k], b[0][n][k]) for n in a[0] for k in GROUPS)


def entry_ranges(m):
    """{group: [(start, end, unit)]}: the segments."""
    out = {}
    for g in GROUPS:
        lay = m.layout(g)
        out[g] = [(off, off + r * c, i // 2) for i, (_, off, r, c) in enumerate(lay)]
        assert out[g][-1][1] == m.group_size(g)
    return out


def unit_mask(m, pick):
    """{group: bool[n]}: the elements of the units for which pick(global unit number, name) holds."""
    rng = entry_ranges(m)
    number = {(g, i): k for k, (_, g, i) in enumerate(m.layers())}
    name = {(g, i): n for n, g, i in m.layers()}
    out = {}
    for g in GROUPS:
        out[g] = np.zeros(m.group_size(g), bool)
        for a, b, u in rng[g]:
            out[g][a:b] = bool(pick(number[(g, u)], name[(g, u)]))
    return out


def test_the_layouts_have_the_boundaries_the_tests_rely_on():
    m, e = new_model(util.SMALL), new_model(util.EDGE)
    ends = [b for _, b, _ in entry_ranges(m)["mult"]]
    assert 5941 in ends and sum(b % 2 for b in ends) > 10          # odd offsets behind attscore
    r = entry_ranges(e)["mult"]
    assert any(b - a == 1 for a, b, _ in r)                         # one-float biases
    spans = [len([1 for a, b, _ in r if a < q + 4 and b > q]) for q in range(0, r[-1][1], 4)]
    assert sum(s >= 2 for s in spans) >= 10                         # quads that span segments
    assert len(m.layers()) == 18 and [len(entry_ranges(m)[g]) for g in GROUPS] == [1, 8, 26]
    m.close()
    e.close()


# ------------------------------------------------------------------ 1. defaults: rau_update's bits
def _defaults(dims, params, grad_steps, combos, null_extras=False):
    a, b = new_model(dims, params), new_model(dims, params)
    if params is None:
        b.set_params(a.get_params())
    p0 = a.get_params()
    for rule, scope in combos:
        for m in (a, b):
            m.set_params(p0)
            m.reset_opt_state(rule)
        for t, grads in enumerate(grad_steps):
            a.set_grads(grads)
            b.set_grads(grads)
            o = opts(rule, scope, eta=0.01, noise_seed=7)
            rca, na = plain(a, t, o)
            rcb, nb = ex(b, t, o, null_extras=null_extras)
            assert rca == 0 and rcb == 0
            assert same_bits(na, nb), (rule, scope, t, na, nb)
            assert same_state(state(a), state(b)), (rule, scope, t)
    a.close()
    b.close()


def test_defaults_give_rau_updates_bits(prob):
    dims, params, grads = prob
    _defaults(dims, params, grads, RULE_SCOPE)
    _defaults(dims, params, grads[:1], RULE_SCOPE[:1], null_extras=True)


def test_defaults_give_rau_updates_bits_beyond_a_million_floats():
    """embed and mult exceed one million floats: every grid-stride loop wraps, all 1024 partials are in use."""
    m = new_model(BIG)
    sizes = m.group_sizes()
    m.close()
    assert sizes["mult"] > 1_000_000 and sizes["embed"] > 1_000_000
    rng = np.random.default_rng(8)
    grads = {k: (rng.standard_normal(n) * 0.01).astype(np.float32) for k, n in sizes.items()}
    _defaults(BIG, None, [grads], [("adam", "global"), ("adamax", "group")])


# ------------------------------------------------------------------ 2. scales, bitwise
def test_power_of_two_scales_are_halved_step_sizes_segment_by_segment(prob):
    dims, params, grads = prob
    lr, mult_lr = 3e-3, 3e-4
    for rule, scope in (("adam", "group"), ("adamax", "global")):
        full, half, all_half, mixed = (new_model(dims, params) for _ in range(4))
        all_half.set_layer_opts("*", lr_scale=0.5)
        for k, (name, _, _) in enumerate(mixed.layers()):
            if k % 2:
                mixed.set_layer_opts(name, lr_scale=0.5)
        halved = unit_mask(mixed, lambda k, name: k % 2 == 1)
        assert all(v.any() and not v.all() for g, v in halved.items() if g != "embed")
        for t in range(3):
            for m in (full, half, all_half, mixed):
                m.set_grads(grads[t])
            kw = dict(eta=0.01, noise_seed=11)
            _, n_full = plain(full, t, opts(rule, scope, lr=lr, mult_lr=mult_lr, **kw))
            _, n_half = plain(half, t, opts(rule, scope, lr=lr / 2, mult_lr=mult_lr / 2, **kw))
            rc1, n_all = ex(all_half, t, opts(rule, scope, lr=lr, mult_lr=mult_lr, **kw))
            rc2, n_mix = ex(mixed, t, opts(rule, scope, lr=lr, mult_lr=mult_lr, **kw))
            assert rc1 == 0 and rc2 == 0
            assert same_bits(n_full, n_half) and same_bits(n_full, n_all) and same_bits(n_full, n_mix)
            sf, sh, sa, sm = (state(m) for m in (full, half, all_half, mixed))
            assert same_state(sh, sa), (rule, t)                       # all 0.5 == lr / 2
            for name in ("g", "m", "v"):                               # no step size in them: equal in every run
                assert all(same_bits(sf[0][name][k], sm[0][name][k]) for k in GROUPS), (rule, t, name)
            for k in GROUPS:                                           # x: element by element, by its segment
                want = np.where(halved[k], bits(sh[0]["x"][k]), bits(sf[0]["x"][k]))
                bad = np.flatnonzero(bits(sm[0]["x"][k]) != want)
                assert bad.size == 0, (rule, t, k, bad[:8])
                assert not same_bits(sf[0]["x"][k], sh[0]["x"][k])     # the two runs do differ
        for m in (full, half, all_half, mixed):
            m.close()


# ------------------------------------------------------------------ 3. frozen
def _freeze_some(m):
    """Every third layer, the one-float-bias layers and the embedding among them."""
    names = [n for k, (n, _, _) in enumerate(m.layers()) if k % 3 == 0 or n.endswith(("attscore", "out_do_pred"))]
    m.freeze(*names)
    return unit_mask(m, lambda k, n: n in names)


def test_frozen_layers_keep_their_bits_and_leave_the_norms(prob):
    dims, params, grads = prob
    rng = np.random.default_rng(5)
    for rule, scope in (("adam", "global"), ("adamax", "group")):
        a, c = new_model(dims, params), new_model(dims, params)
        o = opts(rule, scope, eta=0.0)
        for m in (a, c):                                    # one step first: non-zero moments
            m.set_grads(grads[0])
        assert plain(a, 0, o)[0] == 0 and ex(c, 0, o)[0] == 0
        frozen = _freeze_some(c)
        assert frozen["embed"].all() and all(v.any() and not v.all() for g, v in frozen.items() if g != "embed")
        c.set_ema({k: rng.standard_normal(v.size).astype(np.float32) for k, v in params.items()})
        c.set_grads(grads[1])
        a.set_grads({k: np.where(frozen[k], np.float32(0), grads[1][k]) for k in GROUPS})
        before = state(c)
        rca, na = plain(a, 1, o)
        rcc, nc = ex(c, 1, o, ema_decay=0.9)
        assert rca == 0 and rcc == 0
        assert same_bits(na, nc), (na, nc)                  # zeros add nothing to a sum of squares, in the same order
        sa, sc = state(a), state(c)
        for k in GROUPS:
            f = frozen[k]
            for name in ("x", "g", "m", "v", "e"):
                assert np.array_equal(bits(sc[0][name][k])[f], bits(before[0][name][k])[f]), (rule, k, name)
            for name in ("x", "g", "m", "v"):
                assert np.array_equal(bits(sc[0][name][k])[~f], bits(sa[0][name][k])[~f]), (rule, k, name)
            if (~f).any():
                assert not np.any(bits(sc[0]["e"][k])[~f] == bits(before[0]["e"][k])[~f])   # the rest averaged
        a.close()
        c.close()


def _check_against_ref(got, ref, norms, ref_norms, names):
    for k in GROUPS:
        for name in names:
            a, b = got[name][k], ref[name][k]
            assert np.all(np.isfinite(a)), (k, name)
            err = util.rel_err(a, b) if np.any(b) else float(np.max(np.abs(a)))
            print(f"{k}.{name}: rel_err {err:.2e}")
            assert err < 1e-5, (k, name, err)
    for i in range(4):
        print(f"norm[{i}]: device {norms[i]:.8g} ref {ref_norms[i]:.8g}")
        assert abs(norms[i] - ref_norms[i]) < 1e-5 * max(1.0, ref_norms[i]), i


def _segs(m, opt_of_unit=None):
    """update_ex_ref segments of the model's layout; opt_of_unit: {(group, unit): (lr_scale, decay, bias_decay)}."""
    return {g: update_ex_ref.segments(m.layout(g), {u: v for (gg, u), v in (opt_of_unit or {}).items() if gg == g})
            for g in GROUPS}


def test_frozen_layers_with_noise_match_the_fp64_statement(prob):
    dims, params, grads = prob
    m = new_model(dims, params)
    frozen = _freeze_some(m)
    m.set_grads(grads[0])
    step_t, seed = 5, 77
    rc, norms = ex(m, step_t, opts("adamax", "global", eta=0.01, gamma=0.55, clip=0.1, noise_seed=seed))
    assert rc == 0
    noise = {k: device_normals(params[k].size, seed, step_t, i) for i, k in enumerate(GROUPS)}
    z = {k: np.zeros(v.size) for k, v in params.items()}
    segs = _segs(m, {(g, i): (0.0, 1.0, 0.0) for n, g, i in m.layers() if m.layer_opts()[n][0] == 0.0})
    x, gc, mo, vo, _, ref_norms = update_ex_ref.update(
        {k: v.astype(np.float64) for k, v in params.items()}, grads[0], z, z, None, {k: 1 for k in GROUPS}, step_t,
        segs, noise=noise, rule="adamax", clip_scope="global", eta=0.01, gamma=0.55, clip=0.1)
    got = state(m)[0]
    _check_against_ref(got, {"x": x, "g": gc, "m": mo, "v": vo}, norms, ref_norms, ("x", "g", "m", "v"))
    for k in GROUPS:                                         # and no noise reached a frozen gradient
        assert np.array_equal(bits(got["g"][k])[frozen[k]], bits(grads[0][k])[frozen[k]])
    m.close()


def test_a_whole_group_frozen_has_norm_zero_and_leaves_the_others(small):
    dims, params, grads = small
    a, c = new_model(dims, params), new_model(dims, params)
    c.freeze("rnn.*")
    for m in (a, c):
        m.set_grads(grads[0])
    o = opts("adam", "group", eta=0.01, noise_seed=3)
    _, na = plain(a, 0, o)
    rc, nc = ex(c, 0, o)
    assert rc == 0 and nc[1] == 0.0 and same_bits(na[[0, 2]], nc[[0, 2]])
    assert abs(nc[3] - np.sqrt(float(nc[0]) ** 2 + float(nc[2]) ** 2)) < 1e-5 * max(1.0, float(nc[3]))
    sa, sc = state(a), state(c)
    for name in ("x", "g", "m", "v"):
        assert same_bits(sc[0][name]["embed"], sa[0][name]["embed"]) and \
            same_bits(sc[0][name]["mult"], sa[0][name]["mult"]), name
    assert same_bits(sc[0]["x"]["rnn"], params["rnn"]) and same_bits(sc[0]["g"]["rnn"], grads[0]["rnn"])
    assert not sc[0]["m"]["rnn"].any() and not sc[0]["v"]["rnn"].any()
    a.close()
    c.close()


# ------------------------------------------------------------------ 4. decay and average against fp64
@pytest.mark.parametrize("rule", ["adam", "adamax"])
def test_decay_scales_and_average_match_the_fp64_statement(prob, rule):
    dims, params, grad_steps = prob
    m = new_model(dims, params)
    unit_opts = {}
    for k, (name, g, i) in enumerate(m.layers()):
        unit_opts[(g, i)] = (0.5 + 0.125 * k, 1.0 if k % 4 else 0.5, 1.0 if name.endswith("out_score") else 0.0)
        m.set_layer_opts(name, *unit_opts[(g, i)])
    assert m.layer_opts()["classifier.out_score"][2] == 1.0 and m.layer_opts()["rnn.l1.i2h"][2] == 0.0
    segs = _segs(m, unit_opts)
    m.ema_reset()
    # the statement gets the hyper-parameters the C ABI got: floats.  (1 - float(0.999)) is 1.3e-5 away from 0.001
    f32 = lambda v: float(np.float32(v))
    wd, d = f32(0.1), f32(0.9)
    hyper = dict(lr=f32(3e-3), mult_lr=f32(3e-4), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))
    x = {k: v.astype(np.float64) for k, v in params.items()}
    e = {k: v.copy() for k, v in x.items()}
    mo = {k: np.zeros(v.size) for k, v in params.items()}
    vo = {k: np.zeros(v.size) for k, v in params.items()}
    for t in range(3):
        clip = 1e30 if t == 1 else 0.01                       # step 1: the clip does not engage
        m.set_grads(grad_steps[t])
        rc, norms = ex(m, t, opts(rule, "global", eta=0.0, clip=clip), weight_decay=wd, ema_decay=d)
        assert rc == 0
        x, gc, mo, vo, e, ref_norms = update_ex_ref.update(x, grad_steps[t], mo, vo, e, {k: t + 1 for k in GROUPS}, t,
                                                           segs, rule=rule, clip_scope="global", eta=0.0, clip=clip,
                                                           weight_decay=wd, ema_decay=d, **hyper)
        if t != 1:
            assert ref_norms[3] > clip
        _check_against_ref(state(m)[0], {"x": x, "g": gc, "m": mo, "v": vo, "e": e}, norms, ref_norms,
                           ("x", "m", "v", "e"))
    # the decay did something the bar can see
    nodecay = update_ex_ref.update({k: v.astype(np.float64) for k, v in params.items()}, grad_steps[0],
                                   {k: np.zeros(v.size) for k, v in params.items()},
                                   {k: np.zeros(v.size) for k, v in params.items()}, None, {k: 1 for k in GROUPS}, 0,
                                   segs, rule=rule, clip_scope="global", eta=0.0, clip=0.01)[0]
    first = update_ex_ref.update({k: v.astype(np.float64) for k, v in params.items()}, grad_steps[0],
                                 {k: np.zeros(v.size) for k, v in params.items()},
                                 {k: np.zeros(v.size) for k, v in params.items()}, None, {k: 1 for k in GROUPS}, 0,
                                 segs, rule=rule, clip_scope="global", eta=0.0, clip=0.01, weight_decay=wd)[0]
    assert util.rel_err(first["mult"], nodecay["mult"]) > 1e-5
    m.close()


def test_no_decay_means_the_bits_of_the_run_without(small):
    dims, params, grads = small
    a, b, c = (new_model(dims, params) for _ in range(3))
    for m in (a, b, c):
        m.set_layer_opts("classifier.*", lr_scale=0.75)
        m.set_grads(grads[0])
    c.set_layer_opts("*", decay=0.0, bias_decay=0.0)
    o = opts("adamax", "group", eta=0.01, noise_seed=2)
    ra, na = ex(a, 0, o)                                  # no decay asked for
    rb, nb = ex(b, 0, o, weight_decay=0.0)
    rcc, nc = ex(c, 0, o, weight_decay=0.3)               # asked for, every multiplier 0
    assert (ra, rb, rcc) == (0, 0, 0) and same_bits(na, nb) and same_bits(na, nc)
    assert same_state(state(a), state(b)) and same_state(state(a), state(c))
    b.set_grads(grads[1])
    a.set_grads(grads[1])
    ex(a, 1, o)
    ex(b, 1, o, weight_decay=0.3)                         # and with the default multipliers it does decay
    assert not same_bits(state(a)[0]["x"]["mult"], state(b)[0]["x"]["mult"])
    for m in (a, b, c):
        m.close()


# ------------------------------------------------------------------ 5. the average's life cycle
def test_average_needs_a_reset_and_updates_are_refused_while_swapped(small):
    from rau_vqa_amd._lib import RauError
    dims, params, grads = small
    m = new_model(dims, params)
    m.set_grads(grads[0])
    assert (m.has_ema, m.ema_swapped) == (False, False)
    start = state(m)
    rc, norms = ex(m, 0, opts(), ema_decay=0.9)
    assert rc == STATE and np.all(norms == -1.0) and same_state(start, state(m)) and not m.has_ema
    assert m._lib.rau_ema_swap(m._h) == STATE
    got = np.zeros(params["rnn"].size, np.float32)
    assert m._lib.rau_get_ema(m._h, 1, got.ctypes.data, got.size) == STATE
    m.ema_reset()
    assert m.has_ema and all(same_bits(m.ema()[k], params[k]) for k in GROUPS)
    assert ex(m, 0, opts(eta=0.0), ema_decay=0.9)[0] == 0
    m.set_grads(grads[1])
    held, avg = state(m), m.ema()
    assert all(not same_bits(avg[k], held[0]["x"][k]) for k in GROUPS)
    m.ema_swap()
    assert m.ema_swapped
    assert all(same_bits(m.get_params()[k], avg[k]) for k in GROUPS)          # the readers see the average
    assert all(same_bits(m.ema()[k], held[0]["x"][k]) for k in GROUPS)
    swapped = state(m)
    for call in (lambda: plain(m, 1, opts("adam", "global"))[0], lambda: ex(m, 1, opts())[0],
                 lambda: ex(m, 1, opts(), 0.1, 0.9)[0], lambda: m._lib.rau_ema_reset(m._h),
                 lambda: m._lib.rau_set_ema(m._h, 1, got.ctypes.data, got.size)):
        assert call() == STATE
        assert same_state(swapped, state(m)) and m.ema_swapped
    with pytest.raises(RauError, match="-3"):
        m.update(step_t=1)                                                     # rau_noise_clip_adam
    assert same_state(swapped, state(m))
    m.ema_swap()
    assert not m.ema_swapped and same_state(held, state(m))                    # two swaps restore every bit
    with m.averaged():
        assert m.ema_swapped
    assert not m.ema_swapped and same_state(held, state(m))
    m.set_batch_size(3)                                                        # the average survives a resize
    assert m.has_ema and all(same_bits(m.ema()[k], avg[k]) for k in GROUPS)
    m.close()


def test_forward_under_averaged_is_a_fresh_context_with_the_average():
    dims = util.SMALL
    batch, params, _ = util.make_problem(util.shapes(dims))
    rng = np.random.default_rng(9)
    avg = {k: (v + 0.01 * rng.standard_normal(v.size)).astype(np.float32) for k, v in params.items()}
    m, f = new_model(dims, params), new_model(dims, avg)
    m.set_ema(avg)
    for r in (m, f):
        r.evaluate()
        r.set_batch(batch["feats"], batch["tokens"], batch["lens"], batch["labels"])
    f.forward()
    m.forward()
    trained = (m.losses(), m.logits())
    with m.averaged():
        m.forward()
        assert same_bits(m.losses(), f.losses()) and same_bits(m.logits(), f.logits())
        assert not same_bits(m.logits(), trained[1])
    m.forward()
    assert same_bits(m.losses(), trained[0]) and same_bits(m.logits(), trained[1])
    m.close()
    f.close()


def test_run_resumed_from_a_snapshot_with_the_average_continues_bit_for_bit(small, tmp_path):
    dims, params, grads = small
    a = new_model(dims, params)
    a.freeze("word_embed")
    a.ema_reset()

    def step(m, t):
        m.set_grads(grads[t])
        return m.update(step_t=t, eta=0.01, noise_seed=3, rule="adamax", clip_scope="global", weight_decay=0.05,
                        ema_decay=0.9)
    for t in range(2):
        step(a, t)
    path, bare = str(tmp_path / "resume.t7"), str(tmp_path / "bare.t7")
    a.save_snapshot(path, 2, 0, {"lr": 3e-3}, optim=True, ema=True)
    a.save_snapshot(bare, 2, 0, {"lr": 3e-3}, optim=True)
    b, c = new_model(dims), new_model(dims)
    for m in (b, c):
        m.freeze("word_embed")                            # layer options are the caller's, not the snapshot's
    assert b.load_snapshot(path) == (2, 0, {"lr": 3e-3}) and b.has_ema
    assert c.load_snapshot(bare) == (2, 0, {"lr": 3e-3}) and not c.has_ema
    sa, sb = state(a), state(b)                           # all but the gradients, which a snapshot does not carry
    assert sa[1:] == sb[1:] and all(same_bits(sa[0][n][k], sb[0][n][k]) for n in ("x", "m", "v", "e") for k in GROUPS)
    na, nb = step(a, 2), step(b, 2)
    assert same_bits(na, nb) and same_state(state(a), state(b))
    for m in (a, b, c):
        m.close()


# ------------------------------------------------------------------ 6. launches, determinism
def test_two_launches_per_update_one_per_swap_and_the_same_bits_again(small):
    dims, params, grads = small
    m = new_model(dims, params)
    m.set_layer_opts("classifier.*", lr_scale=0.5)
    m.ema_reset()
    m.set_grads(grads[0])
    m.update(step_t=0, weight_decay=0.1, ema_decay=0.9, noise_seed=4)
    p0, (st0, rule0), e0 = m.get_params(), m.opt_state(), m.ema()
    m.set_grads(grads[1])
    m.sync()
    m.prof_enable(True)
    m.prof_reset()
    n1 = m.update(step_t=1, weight_decay=0.1, ema_decay=0.9, noise_seed=4)
    m.update(step_t=2, rule="adam", clip_scope="global", weight_decay=0.1)     # without the average
    prof = m.prof()
    assert {k: v["launches"] for k, v in prof.items()} == {"upd_ex_sqnorm": 2, "upd_ex_apply": 2}, prof
    m.prof_reset()
    m.ema_swap()
    m.ema_swap()
    assert {k: v["launches"] for k, v in m.prof().items()} == {"ema_swap": 2}
    m.prof_enable(False)
    # back to the state before step 1: the same call gives the same bits
    m.set_params(p0)
    m.set_opt_state(st0, rule0)
    m.set_ema(e0)
    m.set_grads(grads[1])
    ref = new_model(dims, p0)
    ref.set_layer_opts("classifier.*", lr_scale=0.5)
    ref.set_opt_state(st0, rule0)
    ref.set_ema(e0)
    ref.set_grads(grads[1])
    n2 = m.update(step_t=1, weight_decay=0.1, ema_decay=0.9, noise_seed=4)
    n3 = ref.update(step_t=1, weight_decay=0.1, ema_decay=0.9, noise_seed=4)
    assert same_bits(n1, n2) and same_bits(n1, n3) and same_state(state(m), state(ref))
    m.close()
    ref.close()


# ------------------------------------------------------------------ 7. errors
def test_invalid_arguments_change_nothing(small):
    dims, params, grads = small
    m = new_model(dims, params)
    m.set_grads(grads[0])
    m.ema_reset()
    m.set_layer_opts("rnn.l1.h2h", 0.5, 0.25, 0.125)
    start, lo = state(m), m.layer_opts()
    nan, inf = float("nan"), float("inf")
    for group, index, vals in ((1, 1, (-0.5, 1, 0)), (1, 1, (nan, 1, 0)), (1, 1, (inf, 1, 0)), (1, 1, (1, -1, 0)),
                               (1, 1, (1, 1, nan)), (1, 1, (1, 1, -0.1)), (-1, 0, (1, 1, 0)), (3, 0, (1, 1, 0)),
                               (0, 1, (1, 1, 0)), (1, 4, (1, 1, 0)), (2, 13, (1, 1, 0)), (2, -1, (1, 1, 0))):
        assert m._lib.rau_set_layer_opts(m._h, group, index, *vals) == INVALID, (group, index, vals)
        assert m._lib.rau_last_error()
    for group, index in ((-1, 0), (3, 0), (0, 1), (2, 13)):
        assert m._lib.rau_get_layer_opts(m._h, group, index, None, None, None) == INVALID
    assert m.layer_opts() == lo and lo["rnn.l1.h2h"] == (0.5, 0.25, 0.125)
    for kw in (dict(weight_decay=-0.1), dict(weight_decay=nan), dict(weight_decay=inf), dict(ema_decay=-0.1),
               dict(ema_decay=1.0), dict(ema_decay=1.5), dict(ema_decay=nan)):
        rc, norms = ex(m, 0, opts(), **kw)
        assert rc == INVALID and np.all(norms == -1.0), kw
    from rau_vqa_amd import _lib as L
    for step_t, o in ((0, opts(clip=0.0)), (0, opts(gamma=0.0)), (0, opts(eta=-0.01)), (-1, opts())):
        assert ex(m, step_t, o)[0] == INVALID                                  # rau_update's validation of opts
    bad = opts()
    bad.rule = 2
    assert ex(m, 0, bad)[0] == INVALID
    assert m._lib.rau_update_ex(m._h, 0, None, C.byref(L.RauUpdateExtras()), None) == INVALID
    got = np.zeros(5, np.float32)
    assert m._lib.rau_get_ema(m._h, 1, got.ctypes.data, got.size) == INVALID   # a wrong length
    assert m._lib.rau_set_ema(m._h, 1, got.ctypes.data, got.size) == INVALID
    assert m._lib.rau_get_ema(m._h, 3, got.ctypes.data, got.size) == INVALID
    assert same_state(start, state(m))
    # the other rule's state is refused as rau_update refuses it
    assert ex(m, 0, opts("adamax"), weight_decay=0.1)[0] == 0
    m.set_grads(grads[1])
    held = state(m)
    assert ex(m, 1, opts("adam"))[0] == STATE and same_state(held, state(m))
    m.close()
