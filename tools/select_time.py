"""Cost of training the step-selection head in the step-level backward (rau_backward_select), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the
end of the timed window:
  * null_ms      the step with select_w = NULL (rau_backward_select; the launches of rau_backward);
  * select_ms    the step with select_w = 1 on every hop;
  * parent_ms    the step of ANOTHER build of the library given with --parent-lib (the commit before this feature,
                 built by the caller: it is not part of the tree), through rau_backward.
Method: every leg is warmed up, then timed over --steps steps, --rounds times; legs alternate inside one process
(null, select, null, select, ...) and the two libraries alternate as child processes (a library is loaded once
per process).  Reported per leg: the median of the rounds and their spread (max - min).  The condition on the
NULL path: |null_ms - parent_ms| within the parent's own spread.  A last child profiles one select step per
config with the library's per-launch events (rau_prof_enable) and prints the classes the feature adds or moves:
select_signal, select_wgrad and head_dgrad (the two products the select step forms in the backward; a NULL step
forms them in the forward under the same class name).
One JSON line per config:

    python tools/select_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 3] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {1: dict(D=512, dtype="f32"), 2: dict(D=2048, dtype="bf16")}   # bench.py: configs[1], configs[2]


def child(args):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import synth
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=256, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    m.set_batch(**synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123, lens="full"))
    m.training()
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    ones = np.ones(cfg.H, np.float32)
    n = [0]

    def step(leg):
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        if leg == "parent":
            m.backward(hop_w)
        elif leg == "null":
            from rau_vqa_amd._lib import check
            check(m._lib.rau_backward_select(m._h, hop_w.ctypes.data, None))
        else:
            m.backward(hop_w, ones)

    def timed(leg):
        for _ in range(args.warmup):
            step(leg)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(leg)
        m.sync()
        return (time.perf_counter() - t0) / args.steps * 1e3

    out = {}
    if args.leg == "profile":
        for _ in range(args.warmup):
            step("select")
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        step("select")
        m.sync()
        prof = m.prof()
        m.prof_enable(False)
        for name in ("select_signal", "select_wgrad", "head_dgrad", "scale_hops"):
            e = prof.get(name)
            if e:
                out[name] = {"launches": int(e["launches"]), "ms_per_step": round(float(e["ms"]), 4)}
    else:
        legs = ["parent"] if args.leg == "parent" else ["null", "select"]
        out = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print("SELECT_TIME " + json.dumps(out), flush=True)


def run_child(args, config, leg, lib=None):
    env = dict(os.environ)
    if lib:
        env["RAU_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--config", str(config), "--steps",
           str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"child {leg} (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("SELECT_TIME "):
            return json.loads(line[len("SELECT_TIME "):])
    raise SystemExit(f"child {leg} printed no result:\n{p.stdout[-2000:]}")


def summary(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "spread_ms": round(float(max(ts) - min(ts)), 4),
            "rounds": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librau.so of the commit before the feature (optional)")
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2], choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=2, help="child processes per library and config")
    ap.add_argument("--leg", default=None, help="(internal) run one child leg")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    for config in args.configs:
        acc = {"parent": [], "null": [], "select": []}
        for _ in range(args.passes):   # the two libraries alternate
            if args.parent_lib:
                acc["parent"] += run_child(args, config, "parent", args.parent_lib)["parent"]
            r = run_child(args, config, "this")
            acc["null"] += r["null"]
            acc["select"] += r["select"]
        res = {"tool": "select_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps, "null": summary(acc["null"]), "select": summary(acc["select"])}
        res["select_extra_ms"] = round(res["select"]["median_ms"] - res["null"]["median_ms"], 4)
        if args.parent_lib:
            res["parent"] = summary(acc["parent"])
            d = abs(res["null"]["median_ms"] - res["parent"]["median_ms"])
            res["null_minus_parent_ms"] = round(res["null"]["median_ms"] - res["parent"]["median_ms"], 4)
            res["null_inside_parent_spread"] = bool(d <= res["parent"]["spread_ms"])
        res["profile_select_step"] = run_child(args, config, "profile")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
