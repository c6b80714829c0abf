"""Time of rau_layer_stats and of the update guard, one GPU, in the style of tools/update_ex_time.py.

At the parameter sizes of bench.py's configs[1] (Ours_SS, D = 512) and configs[2] (Ours_ResNet, D = 2048):

(a) the readout.  rau_layer_stats (two launches and a download of 35 records) for the gradients, gradients + weights,
    and all three sources, each against the route it replaces: get_grads() (+ get_params(), + opt_state()) and the
    per-layer norms in numpy on the host.  Device legs: --calls calls back to back, one rau_sync at the end; also the
    achieved bytes/s of the first pass from the profile's own events (4 bytes per element and source, 8 more for the
    direction), to set beside l2norm_features' rate.  Host legs: one call per round.
(b) the update.  rau_update with the guard off and on against rau_update of ANOTHER build of the library
    (--parent-lib: the parent commit's librau.so, built in a copy of its own tree), which runs in a process of its
    own before and after this build's legs.  Guard off should sit inside the parent's spread; guard on is one more
    read of the gradients and one stream synchronisation per update, reported, not bounded.
Medians over --rounds rounds, spread = max - min.  One JSON line per config:

    python tools/layer_stats_time.py [--parent-lib PATH] [--configs 1 2] [--calls 50] [--rounds 5] [--warmup 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {1: dict(D=512, dtype="f32"), 2: dict(D=2048, dtype="bf16")}   # bench.py: configs[1], configs[2]
STAT_LEGS = {"stats_grad": (True, False, False), "stats_grad_param": (True, True, False),
             "stats_all": (True, True, True)}
HOST_LEGS = {"host_grad": 1, "host_grad_param": 2, "host_all": 3}
UPDATE_LEGS = ("update_guard_off", "update_guard_on")


def child(args):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import _lib as L
    from rau_vqa_amd import layer_stats as LS
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=8, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    sizes = m.group_sizes()
    floats = int(sum(sizes.values()))
    rng = np.random.default_rng(1)
    grads = {k: (rng.standard_normal(n) * 0.01).astype(np.float32) for k, n in sizes.items()}
    lib, h = m._lib, m._h
    o = L.RauUpdateOpts()
    lib.rau_update_opts_default(C.byref(o))
    n = [0]

    def update():
        L.check(lib.rau_update(h, n[0], C.byref(o), None))
        n[0] += 1

    def timed_update(guard):
        m.reset_opt_state()
        m.set_grads(grads)
        if not args.only_update:
            m.guard_updates(guard)
        for _ in range(args.warmup):
            update()
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            update()
        m.sync()
        return (time.perf_counter() - t0) / args.calls * 1e3

    if args.only_update:
        out = {"update": [round(timed_update(False), 4) for _ in range(args.rounds)]}
        m.close()
        print("LAYER_STATS_TIME " + json.dumps({"floats": floats, **out}), flush=True)
        return

    layouts = {g: m.layout(g) for g in L.GROUPS}

    def timed_stats(leg):
        gr, pa, di = STAT_LEGS[leg]
        for _ in range(args.warmup):
            m.layer_stats_tensor(gr, pa, di)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            m.layer_stats_tensor(gr, pa, di)
        m.sync()
        return (time.perf_counter() - t0) / args.calls * 1e3

    def timed_host(leg):
        k = HOST_LEGS[leg]
        t0 = time.perf_counter()
        g = m.get_grads()
        p = m.get_params() if k >= 2 else None
        mom = {kk: v[:2] for kk, v in m.opt_state()[0].items()} if k >= 3 else None
        LS.stats(layouts, grads=g, params=p, moments=mom)
        return (time.perf_counter() - t0) * 1e3

    def part_rate(leg):
        """bytes/s of layer_stats_part by the profile's events (the launch alone, no host time)"""
        gr, pa, di = STAT_LEGS[leg]
        m.prof_enable(True)
        m.prof_reset()
        for _ in range(args.calls):
            m.layer_stats_tensor(gr, pa, di)
        p = m.prof()["layer_stats_part"]
        f = m.prof()["layer_stats_finish"]
        m.prof_enable(False)
        return {"part_us": round(p["ms"] / p["launches"] * 1e3, 2), "finish_us": round(f["ms"] / f["launches"] * 1e3, 2),
                "part_TBps": round(p["bytes"] / (p["ms"] * 1e-3) / 1e12, 3)}

    m.set_grads(grads)
    update()      # the direction needs moments
    m.set_grads(grads)
    out = {leg: [] for leg in (*STAT_LEGS, *HOST_LEGS, *UPDATE_LEGS)}
    # the update legs first and on their own, as the parent's process runs them: a leg that follows the host legs'
    # 0.1 to 0.3 s of numpy work starts on an idle device, which five warm-up updates do not undo
    for _ in range(args.rounds):
        out["update_guard_off"].append(round(timed_update(False), 4))
        out["update_guard_on"].append(round(timed_update(True), 4))
    m.guard_updates(False)
    for _ in range(args.rounds):
        for leg in STAT_LEGS:
            out[leg].append(round(timed_stats(leg), 4))
        for leg in HOST_LEGS:
            out[leg].append(round(timed_host(leg), 3))
    rates = {leg: part_rate(leg) for leg in STAT_LEGS}
    skipped = m.update_guard["skipped"]
    finite = all(bool(np.all(np.isfinite(a))) for a in m.get_params().values())
    m.close()
    print("LAYER_STATS_TIME " + json.dumps({"floats": floats, "finite": finite, "skipped": skipped, "rates": rates,
                                            **out}), flush=True)


def run_child(args, config, parent_lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", str(config), "--calls", str(args.calls),
           "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    env = dict(os.environ)
    env.pop("RAU_LIB", None)
    if parent_lib:
        cmd.append("--only-update")
        env["RAU_LIB"] = os.path.abspath(parent_lib)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    if p.returncode != 0:
        raise SystemExit(f"child (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("LAYER_STATS_TIME "):
            return json.loads(line[len("LAYER_STATS_TIME "):])
    raise SystemExit(f"child printed no result:\n{p.stdout[-2000:]}")


def summary(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "spread_ms": round(float(max(ts) - min(ts)), 4),
            "rounds": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librau.so of the parent commit: adds the parent_update legs")
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2], choices=sorted(CONFIGS))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="(internal) run one config in this process")
    ap.add_argument("--only-update", action="store_true", help="(internal) the rau_update leg alone")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for config in args.configs:
        res = {"tool": "layer_stats_time", "config": f"configs[{config}]", **CONFIGS[config], "calls": args.calls}
        if args.parent_lib:
            res["parent_update_before"] = summary(run_child(args, config, args.parent_lib)["update"])
        r = run_child(args, config)
        res.update(floats=r["floats"], finite=r["finite"], skipped=r["skipped"], rates=r["rates"])
        for leg in (*STAT_LEGS, *HOST_LEGS, *UPDATE_LEGS):
            res[leg] = summary(r[leg])
        for s, hleg in zip(STAT_LEGS, HOST_LEGS):
            res[f"{hleg}_over_{s}"] = round(res[hleg]["median_ms"] / res[s]["median_ms"], 1)
        if args.parent_lib:
            res["parent_update_after"] = summary(run_child(args, config, args.parent_lib)["update"])
            both = res["parent_update_before"]["rounds"] + res["parent_update_after"]["rounds"]
            res["parent_update"] = base = summary(both)
            d = res["update_guard_off"]["median_ms"] - base["median_ms"]
            res["guard_off_minus_parent_ms"] = round(d, 4)
            res["guard_off_within_parent_spread"] = bool(d <= base["spread_ms"])
        res["guard_on_minus_off_ms"] = round(res["update_guard_on"]["median_ms"] -
                                             res["update_guard_off"]["median_ms"], 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
