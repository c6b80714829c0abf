"""Time of rau_update_ex alone, one GPU, against rau_update (update.hip), in the style of tools/update_time.py.

At the parameter sizes of bench.py's configs[1] (Ours_SS, D = 512) and configs[2] (Ours_ResNet, D = 2048), with
gradient noise on (eta = 0.01), RAU_OPT_ADAM + RAU_CLIP_GROUP, the legs
  * parent_update  rau_update of ANOTHER build of the library (--parent-lib: the parent commit's librau.so, built
                   beside this one), in a process of its own, run before and after this build's legs;
  * update         this build's rau_update: its code path is untouched, so it should sit inside the parent's spread;
  * ex_default     rau_update_ex, extras and every layer at their defaults (rau_update's bits);
  * ex_decay       rau_update_ex with weight_decay = 0.01 and a distinct lr_scale per layer;
  * ex_ema         the same plus the weight average (ema_decay = 0.999): 44 bytes per element instead of 36.
This build's legs alternate inside every round of ONE process.  A leg = reset the optimizer state, warm up, then
--updates updates back to back with no norms read back (no host synchronisation inside the window) and one rau_sync
at its end; reported per leg: the median over --rounds rounds of the time per update, and the spread (max - min).
One JSON line per config:

    python tools/update_ex_time.py [--parent-lib PATH] [--configs 1 2] [--updates 50] [--rounds 5] [--warmup 5]
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
LEGS = ("update", "ex_default", "ex_decay", "ex_ema")


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
    legs = ("update",) if args.only_update else LEGS
    n = [0]

    def layers(scaled):
        for k, (name, _, _) in enumerate(m.layers()):
            m.set_layer_opts(name, lr_scale=(0.5 + 0.05 * k) if scaled else 1.0)

    def update(leg):
        if leg == "update":
            L.check(lib.rau_update(h, n[0], C.byref(o), None))
        else:
            x = L.RauUpdateExtras(weight_decay=0.0 if leg == "ex_default" else 0.01,
                                  ema_decay=0.999 if leg == "ex_ema" else 0.0)
            L.check(lib.rau_update_ex(h, n[0], C.byref(o), C.byref(x), None))
        n[0] += 1

    def timed(leg):
        m.reset_opt_state()
        m.set_grads(grads)
        if not args.only_update:
            layers(leg in ("ex_decay", "ex_ema"))
            if leg == "ex_ema":
                m.ema_reset()
        for _ in range(args.warmup):
            update(leg)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.updates):
            update(leg)
        m.sync()
        return (time.perf_counter() - t0) / args.updates * 1e3

    out = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            out[leg].append(round(timed(leg), 4))
    finite = all(bool(np.all(np.isfinite(a))) for a in m.get_params().values())
    m.close()
    print("UPDATE_EX_TIME " + json.dumps({"floats": int(sum(sizes.values())), "finite": finite, **out}), flush=True)


def run_child(args, config, parent_lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", str(config), "--updates",
           str(args.updates), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    env = dict(os.environ)
    env.pop("RAU_LIB", None)
    if parent_lib:
        cmd.append("--only-update")
        env["RAU_LIB"] = os.path.abspath(parent_lib)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    if p.returncode != 0:
        raise SystemExit(f"child (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("UPDATE_EX_TIME "):
            return json.loads(line[len("UPDATE_EX_TIME "):])
    raise SystemExit(f"child printed no result:\n{p.stdout[-2000:]}")


def summary(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "spread_ms": round(float(max(ts) - min(ts)), 4),
            "rounds": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librau.so of the parent commit: adds the parent_update legs")
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2], choices=sorted(CONFIGS))
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="(internal) run one config in this process")
    ap.add_argument("--only-update", action="store_true", help="(internal) the rau_update leg alone")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    for config in args.configs:
        res = {"tool": "update_ex_time", "config": f"configs[{config}]", **CONFIGS[config], "updates": args.updates}
        if args.parent_lib:
            res["parent_update_before"] = summary(run_child(args, config, args.parent_lib)["update"])
        r = run_child(args, config)
        res.update(floats=r["floats"], finite=r["finite"])
        for leg in LEGS:
            res[leg] = summary(r[leg])
        if args.parent_lib:
            res["parent_update_after"] = summary(run_child(args, config, args.parent_lib)["update"])
            both = res["parent_update_before"]["rounds"] + res["parent_update_after"]["rounds"]
            res["parent_update"] = summary(both)
            base = res["parent_update"]
        else:
            base = res["update"]
        for leg in LEGS:
            d = res[leg]["median_ms"] - base["median_ms"]
            res[f"{leg}_minus_base_ms"] = round(d, 4)
            res[f"{leg}_within_base_spread"] = bool(d <= base["spread_ms"])
        res["ex_ema_over_base"] = round(res["ex_ema"]["median_ms"] / base["median_ms"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
