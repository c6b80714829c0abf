"""rau_layer_stats on the device against its numpy statement (rau_vqa_amd/layer_stats.py).

Bars.  sumsq: relative error against the float64 sum of the same squares at most layer_stats.bar(n) = (L(n) + 2) 2^-24,
derived from the summation order layer_stats.hip states, not measured.  absmax and nonfinite: exact.  The direction is
formed in float32 with one rounding per operation on both sides, so its absmax is exact as well.

Shapes.  util.EDGE, util.SMALL, util.MEDIUM: their MULT entries start behind attscore's one-element bias at offsets
that are 1 mod 4 and have biases of 1 and 4 elements; MEDIUM's largest entries span several items at such offsets.
Every width but S and K is a multiple of 4, so the other two remainders come from S: util.SMALL with S = 13 puts the
entries behind attbymemory at offsets 2 mod 4, with S = 14 at 3 mod 4.
Four more are util.SMALL with another word_embed [V, E].  E must be a multiple of 4, so V E is one too:
  below   V E = 8188 = 2047 x 4   CHUNK - 1 = 8191 is prime; 8188 is the nearest product on that side of the boundary
  at      V E = 8192 = 2048 x 4   CHUNK
  above   V E = 8196 = 2049 x 4   CHUNK + 1 = 8193 = 3 x 2731 has no factor that is a multiple of 4; the nearest above
  three   V E = 16400 = 4100 x 4  more than 2 CHUNK: the entry spans three items
Every test prints the largest error / bar it saw (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from rau_vqa_amd import _lib as L
from rau_vqa_amd import layer_stats as LS
from tests import util

pytestmark = pytest.mark.gpu

KEYS = ("B", "T", "V", "E", "Rq", "D", "S", "M", "A", "R", "K", "H")
GROUPS = ("embed", "rnn", "mult")
SHAPES = {
    "edge": util.shapes(util.EDGE), "small": util.shapes(util.SMALL), "medium": util.shapes(util.MEDIUM),
    "below": util.shapes(util.SMALL, V=2047, E=4), "at": util.shapes(util.SMALL, V=2048, E=4),
    "above": util.shapes(util.SMALL, V=2049, E=4), "three": util.shapes(util.SMALL, V=4100, E=4),
    "rem2": util.shapes(util.SMALL, S=13), "rem3": util.shapes(util.SMALL, S=14),
}
REM = {"edge": 1, "small": 1, "medium": 1, "rem2": 2, "rem3": 3}   # offset mod 4 of the entries the shape is there for
INVALID, STATE = -1, -3
SOURCES = ("grad", "param", "dir")


def new_model(sh):
    from rau_vqa_amd.model import RAU, Config
    return RAU(Config(**{k: getattr(sh, k) for k in KEYS}))


def entry_scaled(rng, layouts, sizes, positive=False):
    """{group: vector}: N(0, 1) times a per-entry scale drawn log-uniformly from 1e-6 .. 1e3."""
    out = {}
    for g in GROUPS:
        v = rng.standard_normal(sizes[g])
        for _, a, b in LS.entry_ranges(layouts[g], sizes[g]):
            v[a:b] *= 10.0 ** rng.uniform(-6, 3)
        out[g] = (np.abs(v) if positive else v).astype(np.float32)
    return out


class Case:
    """One shape's model with random gradients, weights and moments in it; the reference is computed once."""

    def __init__(self, name):
        self.name = name
        self.m = new_model(SHAPES[name])
        self.layouts = {g: self.m.layout(g) for g in GROUPS}
        self.sizes = self.m.group_sizes()
        rng = np.random.default_rng(11)
        self.grads = entry_scaled(rng, self.layouts, self.sizes)
        self.params = entry_scaled(rng, self.layouts, self.sizes)
        self.mom = entry_scaled(rng, self.layouts, self.sizes)
        root = entry_scaled(rng, self.layouts, self.sizes, positive=True)
        self.v = {"adam": {g: (root[g] * root[g] + np.float32(1e-30)).astype(np.float32) for g in GROUPS},
                  "adamax": {g: (root[g] + np.float32(1e-12)).astype(np.float32) for g in GROUPS}}
        self.m.set_grads(self.grads)
        self.m.set_params(self.params)
        self.rule = None
        self._ref = {}

    def use_rule(self, rule):
        if self.rule != rule:
            self.m.set_opt_state({g: (self.mom[g], self.v[rule][g], 1) for g in GROUPS}, rule=rule)
            self.rule = rule

    def ref(self, rule, eps):
        if (rule, eps) not in self._ref:
            self._ref[(rule, eps)] = LS.stats(self.layouts, grads=self.grads, params=self.params,
                                              moments={g: (self.mom[g], self.v[rule][g]) for g in GROUPS},
                                              rule=rule, eps=eps)
        return self._ref[(rule, eps)]


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request):
    c = Case(request.param)
    yield c
    c.m.close()


@pytest.fixture(scope="module")
def small():
    c = Case("small")
    yield c
    c.m.close()


def compare(got, want, sources, tag):
    """Every entry, every source: counts and absmax exact, sumsq inside bar(n).  Returns the largest error / bar."""
    assert [(r["name"], r["group"], r["n"]) for r in got] == [(r["name"], r["group"], r["n"]) for r in want]
    worst = 0.0
    for r, w in zip(got, want):
        for s in SOURCES:
            if s not in sources:
                assert s not in r
                continue
            where = (tag, r["name"], s)
            assert r[s]["nonfinite"] == w[s]["nonfinite"], where
            assert np.float32(r[s]["absmax"]) == np.float32(w[s]["absmax"]), where
            assert not np.signbit(r[s]["absmax"]), where
            err = abs(float(r[s]["sumsq"]) - w[s]["sumsq"])
            bar = LS.bar(r["n"]) * w[s]["sumsq"]
            assert err <= bar, (where, err, bar)
            if bar > 0:
                worst = max(worst, err / bar)
            assert r[s]["norm"] == float(np.sqrt(np.float64(r[s]["sumsq"]))), where
    print(f"layer_stats {tag}: largest error / bar = {worst:.3f}")
    return worst


def raw_bits(m, what, eps=1e-8):
    n = m._lib.rau_layer_stats_count(m._h)
    rec = (L.RauLayerStat * n)()
    L.check(m._lib.rau_layer_stats(m._h, what, eps, rec))
    return bytes(rec)


def test_the_shapes_have_the_boundaries_the_tests_rely_on(case):
    lay, n = case.layouts, case.sizes
    embed = n["embed"]
    want = {"below": LS.CHUNK - 4, "at": LS.CHUNK, "above": LS.CHUNK + 4, "three": 2 * LS.CHUNK + 16}
    if case.name in want:
        assert embed == want[case.name] and len(LS.items_of(0, embed)) == {"below": 1, "at": 1, "above": 2,
                                                                          "three": 3}[case.name]
    assert case.m._lib.rau_layer_stats_count(case.m._h) == sum(len(lay[g]) for g in GROUPS) == 35
    if case.name in REM:
        r = LS.entry_ranges(lay["mult"], n["mult"])
        assert REM[case.name] in {a % 4 for _, a, _ in r}            # offsets that are not multiples of 4
        assert any(b - a == 1 for _, a, b in r)                      # a one-element bias
    if case.name == "edge":
        assert any(b - a == 4 for _, a, b in LS.entry_ranges(lay["mult"], n["mult"]))
    if case.name == "medium":
        big = [(a, b) for _, a, b in LS.entry_ranges(lay["mult"], n["mult"]) if b - a > 2 * LS.CHUNK and a % 4]
        assert big                                                   # several items at a misaligned offset


@pytest.mark.parametrize("rule", ["adam", "adamax"])
def test_parity_of_each_source_alone_and_of_all_three(case, rule):
    eps = 1e-8
    case.use_rule(rule)
    want = case.ref(rule, eps)
    m = case.m
    asks = [dict(grads=True, params=False, direction=False), dict(grads=False, params=True, direction=False),
            dict(grads=False, params=False, direction=True), dict(grads=True, params=True, direction=True)]
    got = [m.layer_stats(eps=eps, **a) for a in asks]
    worst = 0.0
    for a, g in zip(asks, got):
        src = [s for s, k in zip(SOURCES, ("grads", "params", "direction")) if a[k]]
        worst = max(worst, compare(g, want, src, f"{case.name}/{rule}/{'+'.join(src)}"))
    # a source's bits do not depend on which other sources were asked for
    for k, s in enumerate(SOURCES):
        for alone, both in zip(got[k], got[3]):
            for f in ("sumsq", "absmax"):
                assert np.float32(alone[s][f]).tobytes() == np.float32(both[s][f]).tobytes(), (alone["name"], s, f)
            assert alone[s]["nonfinite"] == both[s]["nonfinite"]
    assert worst <= 1.0


def poison(vecs, spots):
    out = {g: v.copy() for g, v in vecs.items()}
    for g, i, val in spots:
        out[g][i] = val
    return out


def placement_spots(case):
    """(group, index, value): the first and last element of entries, one-element biases, the scalar head and tail of
    entries at offsets 1, 2 and 3 mod 4, and the two sides of an item boundary where an entry has one."""
    vals = [np.nan, np.inf, -np.inf]
    spots, k = [], 0
    for g in GROUPS:
        for _, a, b in LS.entry_ranges(case.layouts[g], case.sizes[g]):
            idx = {a, b - 1}                                # first and last (the same element in a 1-element bias)
            if b - a > LS.CHUNK:
                idx |= {a + LS.CHUNK - 1, a + LS.CHUNK}     # last element of an item, first of the next
            for i in sorted(idx):
                spots.append((g, i, vals[k % 3]))
                k += 1
    return spots


def test_non_finite_elements_wherever_the_kernel_changes_path(case):
    spots = placement_spots(case)
    r = LS.entry_ranges(case.layouts["mult"], case.sizes["mult"])
    if case.name in REM:      # an entry with a scalar head of 4 - rem elements, a middle and a scalar tail
        assert any(a % 4 == REM[case.name] and b % 4 != 0 and b - a > 8 for _, a, b in r)
        assert any(b - a == 1 for _, a, b in r)
    if case.name == "three":
        assert ("embed", LS.CHUNK - 1) in {(g, i) for g, i, _ in spots}
        assert ("embed", LS.CHUNK) in {(g, i) for g, i, _ in spots}
    m, rule, eps = case.m, "adam", 1e-8
    grads, params, mom = poison(case.grads, spots), poison(case.params, spots[::2]), poison(case.mom, spots[1::2])
    m.set_grads(grads)
    m.set_params(params)
    m.set_opt_state({g: (mom[g], case.v[rule][g], 1) for g in GROUPS}, rule=rule)
    case.rule = None
    try:
        got = m.layer_stats(grads=True, params=True, direction=True, eps=eps)
        want = LS.stats(case.layouts, grads=grads, params=params,
                        moments={g: (mom[g], case.v[rule][g]) for g in GROUPS}, rule=rule, eps=eps)
        assert sum(w["grad"]["nonfinite"] for w in want) == len(spots)
        assert compare(got, want, SOURCES, f"{case.name}/placement") <= 1.0
        # one poisoned element at a time in the one-element bias: the neighbours' records keep every bit
        clean = case.ref(rule, eps)
        a = next(a for _, a, b in r if b - a == 1)
        one = poison(case.grads, [("mult", a, np.nan)])
        m.set_grads(one)
        alone = m.layer_stats()
        for row, w in zip(alone, clean):
            hit = row["group"] == "mult" and row["name"] == next(n for n, s, _ in r if s == a)
            assert row["grad"]["nonfinite"] == (1 if hit else 0), row["name"]
            if hit:
                assert row["grad"]["sumsq"] == 0 and row["grad"]["absmax"] == 0
            else:
                assert abs(float(row["grad"]["sumsq"]) - w["grad"]["sumsq"]) <= LS.bar(row["n"]) * w["grad"]["sumsq"]
    finally:
        m.set_grads(case.grads)
        m.set_params(case.params)


def test_same_bits_on_every_call_and_in_the_device_view(case):
    import torch
    case.use_rule("adam")
    m = case.m
    what = L.STAT_GRAD | L.STAT_PARAM | L.STAT_DIR
    a, b = raw_bits(m, what), raw_bits(m, what)
    assert a == b
    t = m.layer_stats_tensor(grads=True, params=True, direction=True)
    m.sync()
    host = m.layer_stats(grads=True, params=True, direction=True)
    sumsq, absmax = t["sumsq"].cpu().numpy(), t["absmax"].cpu().numpy()
    nonfinite, n = t["nonfinite"].cpu().numpy(), t["n"].cpu().numpy()
    assert t["nonfinite"].dtype == torch.int64 and sumsq.shape == (35, 3)
    for i, row in enumerate(host):
        assert n[i] == row["n"]
        for k, s in enumerate(SOURCES):
            assert sumsq[i, k].tobytes() == np.float32(row[s]["sumsq"]).tobytes()
            assert absmax[i, k].tobytes() == np.float32(row[s]["absmax"]).tobytes()
            assert nonfinite[i, k] == row[s]["nonfinite"]
    # a source that was not asked for leaves zeros
    rec = np.frombuffer(raw_bits(m, L.STAT_PARAM), np.uint32).reshape(35, 14)
    assert not rec[:, [0, 2, 3, 5]].any() and not rec[:, [6, 7, 10, 11]].any() and rec[:, 1].all()


def test_after_a_real_step_the_gradients_agree_with_the_statement(small):
    m = small.m
    sh = util.shapes(util.SMALL)
    batch, params, _ = util.make_problem(sh)
    m.set_params(params)
    try:
        m.training()
        m.set_dropout_seed(7, 3)
        m.set_batch(**batch)
        m.zero_grads()
        m.forward()
        m.backward(np.full(sh.H, float(sh.H), np.float32))
        got = m.layer_stats()
        want = LS.stats(small.layouts, grads=m.get_grads())
        assert any(w["grad"]["sumsq"] > 0 for w in want)
        assert compare(got, want, ["grad"], "small/step") <= 1.0
    finally:
        m.set_params(small.params)
        m.set_grads(small.grads)


def launches(m):
    return {k: v["launches"] for k, v in m.prof().items() if v["launches"]}


def test_refusals_launch_nothing_and_a_clean_call_has_two_launches():
    m = new_model(SHAPES["small"])
    m.init_uniform(seed=1)
    n = m._lib.rau_layer_stats_count(m._h)
    rec = (L.RauLayerStat * n)()
    dev = C.c_void_p()
    m.prof_enable(True)
    m.prof_reset()
    lib = m._lib
    # the direction before any update: no moments
    assert lib.rau_layer_stats(m._h, L.STAT_DIR, 1e-8, rec) == STATE
    assert lib.rau_layer_stats_dev(m._h, L.STAT_GRAD | L.STAT_DIR, 1e-8, C.byref(dev)) == STATE
    assert b"t = 0" in lib.rau_last_error()
    for what in (0, 8, 9, -1, 16):
        assert lib.rau_layer_stats(m._h, what, 1e-8, rec) == INVALID, what
    for eps in (-1e-8, float("nan"), float("inf")):
        assert lib.rau_layer_stats(m._h, L.STAT_GRAD, eps, rec) == INVALID, eps
        assert lib.rau_layer_stats_dev(m._h, L.STAT_DIR, eps, C.byref(dev)) == INVALID, eps
    assert lib.rau_layer_stats(m._h, L.STAT_GRAD, 1e-8, None) == INVALID
    assert launches(m) == {}
    with pytest.raises(ValueError):
        m.layer_stats(grads=False)
    # a clean call: exactly the two launches, under their names
    m.layer_stats(grads=True, params=True)
    assert launches(m) == {"layer_stats_part": 1, "layer_stats_finish": 1}
    m.prof_enable(False)
    m.close()


def test_update_ratios_are_the_last_steps_relative_size():
    m = new_model(SHAPES["small"])
    m.init_uniform(seed=1)
    rng = np.random.default_rng(5)
    grads = {g: (rng.standard_normal(n) * 0.01).astype(np.float32) for g, n in m.group_sizes().items()}
    hyper = dict(lr=3e-3, mult_lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)
    m.set_layer_opts("classifier*", lr_scale=0.5)
    frozen = m.freeze(m.layers()[1][0])
    x0 = m.get_params()
    m.set_grads(grads)
    m.update(0, eta=0.0, clip=1e9, rule="adam", clip_scope="global", **hyper)
    x1 = m.get_params()
    ratios = m.update_ratios(rule="adam", **hyper)
    assert list(ratios) == [name for name, _, _ in m.layers()]
    lay = {g: m.layout(g) for g in GROUPS}
    for name, g, i in m.layers():
        ents = LS.entry_ranges(lay[g], x1[g].size)[2 * i:2 * i + 2]
        a, b = ents[0][1], ents[-1][2]
        dx = (x1[g][a:b].astype(np.float64) - x0[g][a:b].astype(np.float64))
        want = np.linalg.norm(dx) / np.linalg.norm(x1[g][a:b].astype(np.float64))
        if name in frozen:
            assert ratios[name] == 0.0 and want == 0.0
        else:
            # x1 - x0 carries the rounding of x1 (2^-24 |x| per element against steps of 3e-4 .. 3e-3 |x|-ish)
            assert ratios[name] == pytest.approx(want, rel=2e-3), name
    m.set_params({g: np.zeros_like(v) if g == "embed" else v for g, v in x1.items()})
    assert m.update_ratios(rule="adam", **hyper)["word_embed"] == float("inf")
    m.close()
