"""rau_update (Adam / Adamax, group / global clip), the optimizer state's way in and out, rau_dev_adamax.

Bars: bit equality wherever two device paths state the same arithmetic; against the fp64 statement
(tests/update_ref.py) the bars tests/test_update.py applies to the f32 device: util.rel_err < 1e-5 on
weights and moments, 1e-5 * max(1, n) on norms."""
import ctypes as C

import numpy as np
import pytest

from tests import update_ref, util
from tests.test_update import device_normals

pytestmark = pytest.mark.gpu

GROUPS = update_ref.GROUPS
KEYS = ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")
BIG = dict(B=4, T=4, V=6000, E=200, Rq=64, D=64, S=196, M=512, A=256, R=512, K=1000, H=2)   # test_update.py's
INVALID, STATE = -1, -3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def new_model(dims=util.SMALL, params=None):
    from rau_vqa_amd.model import RAU, Config
    m = RAU(Config(**{k: dims[k] for k in KEYS}))
    if params is None:
        m.init_uniform(seed=1)
    else:
        m.set_params(params)
    return m


@pytest.fixture(scope="module")
def small():
    """SMALL parameters and three steps' gradients (0.01 * randn: a clip of 0.1 engages); read-only."""
    _, params, _ = util.make_problem(util.shapes(util.SMALL))
    rng = np.random.default_rng(3)
    grads = [{k: (rng.standard_normal(v.size) * 0.01).astype(np.float32) for k, v in params.items()}
             for _ in range(3)]
    return params, grads


def opts(rule="adam", scope="group", **kw):
    from rau_vqa_amd import _lib as L
    o = L.RauUpdateOpts()
    L.lib().rau_update_opts_default(C.byref(o))
    o.rule = rule if isinstance(rule, int) else L.OPT_RULES[rule]
    o.clip_scope = scope if isinstance(scope, int) else L.CLIP_SCOPES[scope]
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def raw_update(m, step_t, o):
    """rau_update itself (RAU.update routes the default rule and scope to the old call): (rc, norms[4])."""
    norms = np.full(4, -1.0, np.float32)
    rc = m._lib.rau_update(m._h, step_t, C.byref(o), norms.ctypes.data)
    return rc, norms


def snapshot(m):
    """Every buffer an update reads or writes: parameters, gradients, moments, counts, rule."""
    st, rule = m.opt_state()
    return m.get_params(), m.get_grads(), st, rule


def same_snapshot(a, b):
    pa, ga, sa, ra = a
    pb, gb, sb, rb = b
    return ra == rb and all(same_bits(pa[k], pb[k]) and same_bits(ga[k], gb[k]) and sa[k][2] == sb[k][2] and
                            same_bits(sa[k][0], sb[k][0]) and same_bits(sa[k][1], sb[k][1]) for k in GROUPS)


# ------------------------------------------------------------------ 1. same bits as the old call
def _same_bits_as_old(dims, params, grad_steps):
    a, b = new_model(dims, params), new_model(dims, params)
    if params is None:
        b.set_params(a.get_params())
    for t, grads in enumerate(grad_steps):
        a.set_grads(grads)
        b.set_grads(grads)
        na = a.update(step_t=t, eta=0.01, noise_seed=7)               # rau_noise_clip_adam
        rc, nb = raw_update(b, t, opts("adam", "group", eta=0.01, noise_seed=7))
        assert rc == 0
        assert same_bits(na, nb[:3]), (t, na, nb)
        assert same_snapshot(snapshot(a), snapshot(b)), t
        sq = nb[:3].astype(np.float64) ** 2
        assert abs(nb[3] - np.sqrt(sq.sum())) < 1e-5 * max(1.0, float(nb[3]))
    a.close()
    b.close()


def test_adam_group_gives_the_old_calls_bits(small):
    params, grads = small
    _same_bits_as_old(util.SMALL, params, grads)


def test_adam_group_gives_the_old_calls_bits_beyond_a_million_floats():
    """embed and mult exceed one million floats: every grid-stride loop wraps, all 1024 partials are in use."""
    m = new_model(BIG)
    sizes = m.group_sizes()
    m.close()
    assert sizes["mult"] > 1_000_000 and sizes["embed"] > 1_000_000
    rng = np.random.default_rng(8)
    grads = {k: (rng.standard_normal(n) * 0.01).astype(np.float32) for k, n in sizes.items()}
    _same_bits_as_old(BIG, None, [grads])


# ------------------------------------------------------------------ 2. Adamax, global clip, against fp64
def _check_against_ref(m, ref, norms, ref_norms):
    x, _, mo, vo = ref
    got, (st, rule) = m.get_params(), m.opt_state()
    assert rule == "adamax"
    for i, k in enumerate(GROUPS):
        for name, a, b in (("x", got[k], x[k]), ("m", st[k][0], mo[k]), ("u", st[k][1], vo[k])):
            assert np.all(np.isfinite(a)), (k, name)
            err = util.rel_err(a, b) if np.any(b) else float(np.max(np.abs(a)))
            print(f"{k}.{name}: rel_err {err:.2e}")
            assert err < 1e-5, (k, name, err)
    for i in range(4):
        print(f"norm[{i}]: device {norms[i]:.8g} ref {ref_norms[i]:.8g}")
        assert abs(norms[i] - ref_norms[i]) < 1e-5 * max(1.0, ref_norms[i]), i


def test_adamax_global_clip_matches_the_fp64_statement(small):
    params, grad_steps = small
    m = new_model(util.SMALL, params)
    x = {k: v.astype(np.float64) for k, v in params.items()}
    mo = {k: np.zeros(v.size) for k, v in params.items()}
    vo = {k: np.zeros(v.size) for k, v in params.items()}
    for t in range(3):
        grads = dict(grad_steps[t])
        clip = 1e30 if t == 1 else 0.1                    # step 1: the clip does not engage
        if t == 2:
            grads["rnn"] = np.zeros_like(grads["rnn"])    # a group with a zero gradient: u = max(b2 u, eps)
        m.set_grads(grads)
        norms = m.update(step_t=t, lr=3e-3, mult_lr=3e-4, eta=0.0, clip=clip, rule="adamax", clip_scope="global")
        x, gc, mo, vo, ref_norms = update_ref.update(x, grads, mo, vo, {k: t + 1 for k in GROUPS}, t, rule="adamax",
                                                     clip_scope="global", eta=0.0, clip=clip)
        if t != 1:
            assert ref_norms[3] > clip                     # the clip engages
        _check_against_ref(m, (x, gc, mo, vo), norms, ref_norms)
        got_g = m.get_grads()
        for k in GROUPS:                                   # the clipped gradient is written back
            assert np.max(np.abs(got_g[k] - gc[k])) <= 1e-5 * max(np.max(np.abs(gc[k])), 1e-30), k
    m.close()


def test_adamax_global_clip_with_noise_matches_the_fp64_statement(small):
    params, grad_steps = small
    m = new_model(util.SMALL, params)
    m.set_grads(grad_steps[0])
    step_t, seed = 5, 77
    norms = m.update(step_t=step_t, eta=0.01, gamma=0.55, clip=0.1, noise_seed=seed, rule="adamax",
                     clip_scope="global")
    noise = {k: device_normals(params[k].size, seed, step_t, i) for i, k in enumerate(GROUPS)}
    z = {k: np.zeros(v.size) for k, v in params.items()}
    x, gc, mo, vo, ref_norms = update_ref.update({k: v.astype(np.float64) for k, v in params.items()},
                                                 grad_steps[0], z, z, {k: 1 for k in GROUPS}, step_t, noise=noise,
                                                 rule="adamax", clip_scope="global", eta=0.01, gamma=0.55, clip=0.1)
    _check_against_ref(m, (x, gc, mo, vo), norms, ref_norms)
    m.close()


# ------------------------------------------------------------------ 3. resume
def _adamax(m, t, grads):
    m.set_grads(grads)
    return m.update(step_t=t, eta=0.01, noise_seed=3, rule="adamax", clip_scope="global")


def test_resumed_context_continues_bit_for_bit(small, tmp_path):
    params, grads = small
    a = new_model(util.SMALL, params)
    for t in range(2):
        _adamax(a, t, grads[t])
    st, rule = a.opt_state()
    assert rule == "adamax" and all(st[k][2] == 2 for k in GROUPS)
    path = str(tmp_path / "resume.t7")
    a.save_snapshot(path, 2, 0, {"lr": 3e-3}, optim=True)
    b, c, d = (new_model(util.SMALL, a.get_params()) for _ in range(3))
    b.set_opt_state(st, rule)                         # parameters and optimizer state
    assert d.load_snapshot(path) == (2, 0, {"lr": 3e-3})        # the same through a snapshot file
    norms = [_adamax(m, 2, grads[2]) for m in (a, b, c, d)]
    ref = snapshot(a)
    assert same_snapshot(ref, snapshot(b)) and same_bits(norms[0], norms[1])
    assert same_snapshot(ref, snapshot(d)) and same_bits(norms[0], norms[3])
    pc = c.get_params()                               # parameters only: zero moments, t = 1 -- another step
    assert all(not same_bits(pc[k], ref[0][k]) for k in GROUPS)
    assert c.opt_state()[0]["mult"][2] == 1
    for m in (a, b, c, d):
        m.close()


def test_snapshot_without_optim_leaves_the_state_alone(small, tmp_path):
    params, grads = small
    a = new_model(util.SMALL, params)
    _adamax(a, 0, grads[0])
    before = a.opt_state()
    path = str(tmp_path / "plain.t7")
    a.save_snapshot(path, 1, 0, {})
    assert a.load_snapshot(path) == (1, 0, {})
    after = a.opt_state()
    assert after[1] == before[1] == "adamax"
    assert all(same_bits(after[0][k][j], before[0][k][j]) for k in GROUPS for j in (0, 1))
    a.close()


# ------------------------------------------------------------------ 4. state calls
def _set_state(m, group, mv, vv, t, rule):
    return m._lib.rau_set_opt_state(m._h, group, None if mv is None else mv.ctypes.data,
                                    None if vv is None else vv.ctypes.data, t, rule)


def _get_state(m, group, n):
    mv, vv = np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32)
    t, r = C.c_int64(-5), C.c_int32(-5)
    assert m._lib.rau_get_opt_state(m._h, group, mv.ctypes.data, vv.ctypes.data, C.byref(t), C.byref(r)) == 0
    return mv, vv, t.value, r.value


def test_opt_state_calls(small):
    params, _ = small
    m = new_model(util.SMALL, params)
    sizes = m.group_sizes()
    rng = np.random.default_rng(4)
    for gi, k in enumerate(GROUPS):
        n = sizes[k]
        mv, vv, t, r = _get_state(m, gi, n)                      # before any update
        assert not mv.any() and not vv.any() and (t, r) == (0, 0)
        t_only, r_only = C.c_int64(-5), C.c_int32(-5)            # every output may be NULL
        assert m._lib.rau_get_opt_state(m._h, gi, None, None, C.byref(t_only), C.byref(r_only)) == 0
        assert (t_only.value, r_only.value) == (0, 0)
        a, b = rng.standard_normal(n).astype(np.float32), np.abs(rng.standard_normal(n)).astype(np.float32)
        assert _set_state(m, gi, a, b, 9, 1) == 0                # set, then get: the same bits
        mv, vv, t, r = _get_state(m, gi, n)
        assert same_bits(mv, a) and same_bits(vv, b) and (t, r) == (9, 1)
        # RAU_ERR_INVALID, nothing changed: t < 0, t > 0 without both vectors, an unknown rule
        for args in ((a, b, -1, 1), (a, None, 3, 1), (None, b, 3, 1), (None, None, 3, 1), (a, b, 3, 2), (a, b, 3, -1),
                     (None, None, 0, 5)):
            assert _set_state(m, gi, *args) == INVALID, args
            assert m._lib.rau_last_error()
        mv, vv, t, r = _get_state(m, gi, n)
        assert same_bits(mv, a) and same_bits(vv, b) and (t, r) == (9, 1)
        assert _set_state(m, gi, None, None, 0, 0) == 0          # reset: the start state
        mv, vv, t, r = _get_state(m, gi, n)
        assert not mv.any() and not vv.any() and (t, r) == (0, 0)
    for bad_group in (-1, 3):
        assert m._lib.rau_get_opt_state(m._h, bad_group, None, None, None, None) == INVALID
        assert _set_state(m, bad_group, None, None, 0, 0) == INVALID
    m.close()


# ------------------------------------------------------------------ 5. rule ownership, invalid arguments
def test_state_belongs_to_the_rule_that_wrote_it(small):
    from rau_vqa_amd._lib import RauError
    params, grads = small
    m = new_model(util.SMALL, params)
    m.set_grads(grads[0])
    # RAU_ERR_INVALID before anything ran: nothing launched, nothing changed
    start = snapshot(m)
    for step_t, o in ((0, opts(2, "group")), (0, opts(-1, "group")), (0, opts("adam", 2)), (0, opts("adamax", -1)),
                      (0, opts(clip=0.0)), (0, opts(clip=-1.0)), (0, opts(gamma=0.0)), (0, opts(gamma=-0.5)),
                      (0, opts(eta=-0.01)), (-1, opts()), (0, opts("adamax", "global", clip=float("nan")))):
        rc, norms = raw_update(m, step_t, o)
        assert rc == INVALID and np.all(norms == -1.0)
        assert same_snapshot(start, snapshot(m))
    assert m._lib.rau_update(m._h, 0, None, None) == INVALID
    # an Adamax step, then the other rule: RAU_ERR_STATE from both entry points, every bit kept
    rc, _ = raw_update(m, 0, opts("adamax", "global", eta=0.0))
    assert rc == 0
    m.set_grads(grads[1])
    held = snapshot(m)
    assert held[3] == "adamax" and held[2]["embed"][2] == 1
    rc, norms = raw_update(m, 1, opts("adam", "group"))
    assert rc == STATE and np.all(norms == -1.0)
    with pytest.raises(RauError, match="-3"):
        m.update(step_t=1)                                        # rau_noise_clip_adam on Adamax state
    assert same_snapshot(held, snapshot(m))
    # after a reset both run
    m.reset_opt_state()
    assert m.opt_state()[1] == "adam"
    m.update(step_t=1)
    m.set_grads(grads[2])
    rc, _ = raw_update(m, 2, opts("adam", "global"))
    assert rc == 0
    st, rule = m.opt_state()
    assert rule == "adam" and all(st[k][2] == 2 for k in GROUPS)
    rc, _ = raw_update(m, 3, opts("adamax", "group"))             # and Adam's state refuses Adamax
    assert rc == STATE
    m.close()


# ------------------------------------------------------------------ 6. rau_dev_adamax
@pytest.fixture(scope="module")
def dev_ctx():
    m = new_model(util.SMALL)
    yield m
    m.close()


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_dev_adamax_against_the_fp64_statement(dev_ctx, n, misaligned):
    from rau_vqa_amd import modules
    from rau_vqa_amd.modules import DevTensor
    rng = np.random.default_rng(n)
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-8
    off = 1 if misaligned else 0             # a view one float into the allocation: no 16-byte alignment
    base = [DevTensor.zeros(dev_ctx, n + off) for _ in range(4)]
    x, dx, mt, ut = (DevTensor.wrap(dev_ctx, t.ptr + 4 * off, n) for t in base)
    assert (x.ptr % 16 != 0) == misaligned
    x0 = rng.standard_normal(n).astype(np.float32)
    x.copy(x0)
    state = {"t": 0, "m": mt, "u": ut}
    rx, rm, ru = x0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 3):
        g = (rng.standard_normal(n) * 0.01).astype(np.float32)
        if n > 1:
            g[0] = 0.0
        dx.copy(g)
        modules.adamax(x, dx, lr, b1, b2, eps, state)
        assert state["t"] == t
        rx, rm, ru = update_ref.adamax_elem(rx, g.astype(np.float64), rm, ru, t, lr, b1, b2, eps)
        for name, a, b in (("x", x.numpy(), rx), ("m", mt.numpy(), rm), ("u", ut.numpy(), ru)):
            assert np.all(np.isfinite(a))
            assert util.rel_err(a, b) < 1e-5, (name, t)
        assert same_bits(dx.numpy(), g)                         # dx is read only
    if misaligned:                                              # nothing written in front of the views
        assert all(t.numpy()[0] == 0.0 for t in base)


def test_dev_adamax_counts_like_adam_and_equals_the_group_path(small):
    from rau_vqa_amd import modules
    params, grads = small
    a, b = new_model(util.SMALL, params), new_model(util.SMALL, params)
    state = {}
    x, dx = modules.flat(b, "rnn")
    for t in range(2):
        a.set_grads(grads[t])
        b.set_grads(grads[t])
        # no noise and a clip that does not engage: the group path scales by exactly 1
        a.update(step_t=t, lr=3e-3, eta=0.0, clip=1e30, rule="adamax", clip_scope="group")
        modules.adamax(x, dx, 3e-3, state=state)
        assert state["t"] == t + 1 and set(state) == {"t", "m", "u"}
        st, _ = a.opt_state()
        assert same_bits(a.get_params()["rnn"], b.get_params()["rnn"])
        assert same_bits(st["rnn"][0], state["m"].numpy()) and same_bits(st["rnn"][1], state["u"].numpy())
    with pytest.raises(TypeError):
        modules.adamax(x, dx, 3e-3)
    a.close()
    b.close()


# ------------------------------------------------------------------ 7. launch count
def test_two_launches_per_update_under_their_own_names(small):
    params, grads = small
    m = new_model(util.SMALL, params)
    m.set_grads(grads[0])
    m.prof_enable(True)
    m.prof_reset()
    m.update(step_t=0, rule="adamax", clip_scope="global")
    m.update(step_t=1, rule="adamax", clip_scope="group")
    prof = m.prof()
    assert set(prof) <= {"upd_noise_sqnorm", "upd_finish_norm", "upd_apply"}, prof
    assert set(prof) >= {"upd_noise_sqnorm", "upd_apply"}
    assert sum(p["launches"] for p in prof.values()) <= 6
    m.reset_opt_state()
    m.prof_reset()
    m.update(step_t=2)                                            # the old call: nine launches, old names
    prof = m.prof()
    assert {k: v["launches"] for k, v in prof.items()} == {"noise_sqnorm": 3, "finish_norm": 3, "clip_adam": 3}
    m.prof_enable(False)
    m.close()


# ------------------------------------------------------------------ 8. determinism and persistence
def test_same_state_same_bits_and_state_survives_a_resize(small):
    params, grads = small
    m = new_model(util.SMALL, params)
    _adamax(m, 0, grads[0])
    p0, (st0, rule0) = m.get_params(), m.opt_state()
    n1 = _adamax(m, 1, grads[1])
    first = snapshot(m)
    m.set_params(p0)                                              # back to the same state, the same call again
    m.set_opt_state(st0, rule0)
    n2 = _adamax(m, 1, grads[1])
    assert same_snapshot(first, snapshot(m)) and same_bits(n1, n2)
    m.set_batch_size(3)
    st, rule = m.opt_state()
    assert rule == "adamax" and all(st[k][2] == 2 and same_bits(st[k][0], first[2][k][0]) and
                                    same_bits(st[k][1], first[2][k][1]) for k in GROUPS)
    m.set_batch_size(util.SMALL["B"])
    _adamax(m, 2, grads[2])                                       # and the next step is the unresized context's
    ref = new_model(util.SMALL, first[0])
    ref.set_opt_state(first[2], first[3])
    _adamax(ref, 2, grads[2])
    assert same_snapshot(snapshot(m), snapshot(ref))
    m.close()
    ref.close()
