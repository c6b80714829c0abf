"""rau_layer_stats and the update guard without a device: the boundary (header, library, ctypes, Lua), the numpy
statement of the readout (rau_vqa_amd/layer_stats.py) against plain float64 loops, and the chain length L(n) against
the order layer_stats.hip's header states."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from rau_vqa_amd import _lib as L
from rau_vqa_amd import layer_stats as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rau_layer_stats_count", "rau_layer_stats", "rau_layer_stats_dev", "rau_set_update_guard",
         "rau_update_guard")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_calls_the_struct_and_the_constants():
    h = read("include", "rau.h")
    assert re.search(r"#define RAU_ABI_VERSION 5\b", h)
    for name, val in (("RAU_STAT_GRAD", 1), ("RAU_STAT_PARAM", 2), ("RAU_STAT_DIR", 4), ("RAU_GUARD_OFF", 0),
                      ("RAU_GUARD_SKIP", 1)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), h), name
    body = re.search(r"typedef struct rau_layer_stat \{(.*?)\} rau_layer_stat;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    assert [d.split() for d in body.split(";") if d.strip()] == \
        [["float", "sumsq[3]"], ["float", "absmax[3]"], ["int64_t", "nonfinite[3]"], ["int64_t", "n"]]
    code = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    for c in CALLS:
        assert re.search(r"\bint %s\(" % c, code), c
    # the ctypes mirror has the header's layout: 6 floats, 4 int64, no padding
    assert C.sizeof(L.RauLayerStat) == 56 and L.RauLayerStat.nonfinite.offset == 24 and L.RauLayerStat.n.offset == 48
    assert (L.STAT_GRAD, L.STAT_PARAM, L.STAT_DIR, L.GUARD_OFF, L.GUARD_SKIP) == (1, 2, 4, 0, 1)


def test_library_exports_the_calls():
    lib = C.CDLL(L.LIB_PATH)
    for c in CALLS:
        assert hasattr(lib, c), c
        assert c in L._SIGS


def test_null_context_is_refused_without_a_device():
    l = L.lib()
    assert l.rau_layer_stats_count(None) == -1
    assert l.rau_layer_stats(None, 1, 1e-8, None) == -1
    assert l.rau_set_update_guard(None, 1) == -1
    assert l.rau_update_guard(None, None, None, None, None) == -1


def test_lua_binding_carries_the_three_methods():
    lua = read("bindings", "rau.lua")
    for m in ("layerStats", "setUpdateGuard", "updateGuard"):
        assert re.search(r"function RAU:%s\(" % m, lua), m
    for c in CALLS:
        assert re.search(r"\bint %s\(" % c, lua), c


def test_chunk_is_the_kernels_constant():
    k = read("rau_vqa_amd", "csrc", "kernels.h")
    assert int(re.search(r"constexpr int kStatChunk = (\d+);", k).group(1)) == LS.CHUNK


# ---- the numpy statement against plain loops
def loop_stats(x):
    s, a, c = 0.0, 0.0, 0
    for v in x:
        v = float(v)
        if math.isnan(v) or math.isinf(v):
            c += 1
        else:
            s += v * v
            a = max(a, abs(v))
    return s, a, c


LAYOUT = [("a.weight", 0, 3, 5), ("a.bias", 15, 3, 1), ("b.weight", 18, 1, 1), ("b.bias", 19, 1, 1),
          ("c.weight", 20, 7, 9), ("c.bias", 83, 7, 1)]
TOTAL = 90


def test_statement_equals_a_float64_loop_on_a_random_vector():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(TOTAL) * 10.0 ** rng.uniform(-6, 3, TOTAL)).astype(np.float32)
    got = LS.vector_stats(x, LAYOUT)
    assert [g["name"] for g in got] == [e[0] for e in LAYOUT]
    for g, (name, a, b) in zip(got, LS.entry_ranges(LAYOUT, TOTAL)):
        s, m, c = loop_stats(x[a:b])
        assert g["n"] == b - a and g["nonfinite"] == c == 0
        assert g["sumsq"] == pytest.approx(s, rel=1e-14) and float(g["absmax"]) == m


def test_non_finite_elements_at_segment_ends_and_in_a_one_element_segment():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(TOTAL).astype(np.float32)
    x[0], x[14] = np.nan, np.inf             # first and last element of a.weight
    x[15], x[17] = -np.inf, np.nan           # ... of a.bias
    x[18] = np.inf                           # the one-element b.weight
    x[20], x[82] = -np.inf, np.nan           # ... of c.weight
    got = {g["name"]: g for g in LS.vector_stats(x, LAYOUT)}
    assert [got[e[0]]["nonfinite"] for e in LAYOUT] == [2, 2, 1, 0, 2, 0]
    for name, a, b in LS.entry_ranges(LAYOUT, TOTAL):
        s, m, c = loop_stats(x[a:b])
        assert got[name]["nonfinite"] == c and float(got[name]["absmax"]) == m
        assert got[name]["sumsq"] == pytest.approx(s, rel=1e-14)
    assert got["b.weight"]["sumsq"] == 0.0 and float(got["b.weight"]["absmax"]) == 0.0


def test_a_segment_of_nothing_but_nan():
    x = np.ones(TOTAL, np.float32)
    x[20:83] = np.nan
    g = LS.vector_stats(x, LAYOUT)[4]
    assert g["sumsq"] == 0.0 and g["nonfinite"] == 63
    assert float(g["absmax"]) == 0.0 and not np.signbit(g["absmax"])


@pytest.mark.parametrize("rule", [LS.ADAM, LS.ADAMAX])
def test_direction_of_both_rules_against_float64(rule):
    rng = np.random.default_rng(2)
    scale = 10.0 ** rng.uniform(-6, 3, 4000)
    m = (rng.standard_normal(4000) * scale).astype(np.float32)
    v = ((rng.standard_normal(4000) * scale) ** 2 + 1e-30).astype(np.float32) if rule == LS.ADAM else \
        (np.abs(rng.standard_normal(4000)) * scale + 1e-8).astype(np.float32)
    eps = 1e-8
    d = LS.direction(m, v, rule, eps)
    assert d.dtype == np.float32
    m64, v64 = m.astype(np.float64), v.astype(np.float64)
    want = m64 / (np.sqrt(v64) + np.float64(np.float32(eps))) if rule == LS.ADAM else m64 / v64
    # three (Adam) or one (Adamax) rounded operations: (1 + 2^-24)^3 - 1
    assert np.max(np.abs(d - want) / np.abs(want)) <= (3 if rule == LS.ADAM else 1) * 2.0 ** -24 * (1 + 1e-6)
    got = LS.stats({"embed": LAYOUT[:2], "rnn": LAYOUT[:2], "mult": LAYOUT[:2]},
                   moments={g: (m[:18], v[:18]) for g in ("embed", "rnn", "mult")}, rule=rule, eps=eps)
    assert len(got) == 6 and got[0]["dir"]["sumsq"] == pytest.approx(float(np.sum(want[:15] ** 2)), rel=1e-6)
    with pytest.raises(ValueError):
        LS.direction(m, v, "sgd", eps)


# ---- the chain length
def test_chain_length_is_monotone():
    ns = list(range(1, 3000)) + list(range(LS.CHUNK - 600, LS.CHUNK + 600)) + \
        [k * LS.CHUNK + d for k in range(2, 400, 7) for d in (-1, 0, 1, 5)]
    ls = [LS.chain_length(n) for n in sorted(ns)]
    assert all(b >= a for a, b in zip(ls, ls[1:]))
    assert LS.bar(1) == 13 * 2.0 ** -24
    with pytest.raises(ValueError):
        LS.chain_length(0)


def test_chain_length_matches_the_order_the_kernel_file_states():
    ch = LS.CHUNK
    # the values layer_stats.hip's header lists for its formula
    hip = read("rau_vqa_amd", "csrc", "layer_stats.hip")
    assert "L(n) = 4 ceil(floor(c / 4) / 256) + 2  +  8  +  ceil(n / kStatChunk)" in hip
    assert "L(1) = 11, L(255) = L(256) = L(257) = 15" in hip and "L(kStatChunk + 1) = 44" in hip
    want = {1: 11, 255: 15, 256: 15, 257: 15, ch - 1: 43, ch: 43, ch + 1: 44, 3 * ch + 5: 46}
    assert {n: LS.chain_length(n) for n in want} == want
    # ... and counted link by link in that order, at every alignment of the entry's offset: L(n) bounds the count,
    # and is reached wherever an item has a head, a tail and full rounds of quads
    for n in want:
        counted = [LS.longest_chain(off, n) for off in range(4)]
        assert max(counted) <= LS.chain_length(n), (n, counted)
    assert LS.longest_chain(1, ch) == LS.chain_length(ch) == 43
    assert LS.longest_chain(3, 3 * ch + 5) <= 46
    assert LS.items_of(7, 2 * ch + 1) == [(7, ch), (7 + ch, ch), (7 + 2 * ch, 1)]
