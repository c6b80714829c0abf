"""Time of the parameter update alone, one GPU: rau_noise_clip_adam against rau_update (update.hip).

At the parameter sizes of bench.py's configs[1] (Ours_SS, D = 512) and configs[2] (Ours_ResNet, D = 2048) -- the
three flat groups do not depend on the batch size, so the context is created with B = 8 -- and with gradient noise
on (eta = 0.01), three legs in ONE process, alternating inside every round:
  * old_ms           rau_noise_clip_adam: nine launches, 4-byte accesses.  The yardstick: the parent's code,
                     unchanged in this build;
  * adam_ms          rau_update, RAU_OPT_ADAM + RAU_CLIP_GROUP: the same bits in two launches, 16-byte accesses;
  * adamax_global_ms rau_update, RAU_OPT_ADAMAX + RAU_CLIP_GLOBAL.
A leg = reset the optimizer state, warm up, then --updates updates back to back with no norms read back (no host
synchronisation inside the window) and one rau_sync at its end; reported per leg: the median over --rounds rounds
of the time per update, and the spread (max - min) of the rounds.  The expectation from the launch count and the
access width is that the new path is not slower than the old call by more than the old call's own spread.
One JSON line per config:

    python tools/update_time.py [--configs 1 2] [--updates 50] [--rounds 5] [--warmup 5]
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
LEGS = ("old", "adam", "adamax_global")


def child(args):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import _lib as L
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=8, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    sizes = m.group_sizes()
    rng = np.random.default_rng(1)
    grads = {k: (rng.standard_normal(n) * 0.01).astype(np.float32) for k, n in sizes.items()}
    lib, h = m._lib, m._h
    o = L.RauUpdateOpts()
    lib.rau_update_opts_default(C.byref(o))
    n = [0]

    def update(leg):
        if leg == "old":
            L.check(lib.rau_noise_clip_adam(h, n[0], o.lr, o.mult_lr, o.beta1, o.beta2, o.eps, o.eta, o.gamma,
                                            o.clip, 0, None))
        else:
            o.rule = L.OPT_ADAM if leg == "adam" else L.OPT_ADAMAX
            o.clip_scope = L.CLIP_GROUP if leg == "adam" else L.CLIP_GLOBAL
            L.check(lib.rau_update(h, n[0], C.byref(o), None))
        n[0] += 1

    def timed(leg):
        m.reset_opt_state()
        m.set_grads(grads)
        for _ in range(args.warmup):
            update(leg)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.updates):
            update(leg)
        m.sync()
        return (time.perf_counter() - t0) / args.updates * 1e3

    out = {leg: [] for leg in LEGS}
    for _ in range(args.rounds):
        for leg in LEGS:
            out[leg].append(round(timed(leg), 4))
    finite = all(bool(np.all(np.isfinite(a))) for a in m.get_params().values())
    m.close()
    print("UPDATE_TIME " + json.dumps({"floats": int(sum(sizes.values())), "finite": finite, **out}), flush=True)


def run_child(args, config):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", str(config), "--updates",
           str(args.updates), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("UPDATE_TIME "):
            return json.loads(line[len("UPDATE_TIME "):])
    raise SystemExit(f"child printed no result:\n{p.stdout[-2000:]}")


def summary(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "spread_ms": round(float(max(ts) - min(ts)), 4),
            "rounds": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2], choices=sorted(CONFIGS))
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="(internal) run one config in this process")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for config in args.configs:
        r = run_child(args, config)
        res = {"tool": "update_time", "config": f"configs[{config}]", **CONFIGS[config], "floats": r["floats"],
               "updates": args.updates, "finite": r["finite"]}
        for leg in LEGS:
            res[leg] = summary(r[leg])
        for leg in LEGS[1:]:
            d = res[leg]["median_ms"] - res["old"]["median_ms"]
            res[f"{leg}_minus_old_ms"] = round(d, 4)
            res[f"{leg}_not_slower_than_old_spread"] = bool(d <= res["old"]["spread_ms"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
