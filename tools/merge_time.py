"""Cost of training the merged answers in the step-level backward (rau_backward_merged), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the
end of the timed window:
  * parent_ms   the step of ANOTHER build of the library given with --parent-lib (the commit before this
                feature, built by the caller: it is not part of the tree), through rau_backward;
  * null_ms     this build, rau_backward_merged with every optional argument NULL;
  * merged_ms   merge_w = [1, 1]: both merged cross-entropies in the objective.
Method: every leg is warmed up, then timed over --steps steps, --rounds times (five by default); the two legs
of this build alternate inside one process, and the parent runs as a child process of its own BEFORE and AFTER
them (a library is loaded once per process), so that drift over the visit shows in the parent's own numbers.
Reported per leg: the median of the rounds and their spread (max - min).  The condition on the NULL leg:
|null - parent| within the parent's own spread (it is launch for launch the parent's step).  A last child profiles
one merged step per config with the library's per-launch events (rau_prof_enable) and prints the launch the feature
adds (merge_grad) beside the launches around it, with the share of rows on which a hop fired (only those rows
receive the select term).
One JSON line per config:

    python tools/merge_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
LEGS = ("null", "merged")


def child(args):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import synth
    from rau_vqa_amd._lib import check
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=256, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    batch = synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123, lens="full")
    m.set_batch(**batch)
    m.training()
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    ones = np.ones(2, np.float32)
    n = [0]

    def step(leg):
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        if leg == "parent":
            m.backward(hop_w)
        elif leg == "merged":
            m.backward(hop_w, merge_w=ones)
        else:
            check(m._lib.rau_backward_merged(m._h, hop_w.ctypes.data, None, None, None))

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
            step("merged")
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        step("merged")
        m.sync()
        prof = m.prof()
        m.prof_enable(False)
        for name in ("merge_grad", "scale_hops", "head_dgrad", "ce_fwd"):
            e = prof.get(name)
            if e and e["launches"]:
                out[name] = {"launches": int(e["launches"]), "ms_per_step": round(float(e["ms"]), 4)}
        m.forward()
        st = m.step_stats()
        out["step_stats"] = {"loss_uni": round(float(st["loss"][cfg.H]), 4), "loss_select": round(float(st["loss"][cfg.H + 1]), 4),
                             "rows_with_a_firing_hop": int(np.sum(st["selected"])), "rows": cfg.B}
    else:
        legs = ["parent"] if args.leg == "parent" else list(LEGS)
        out = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print("MERGE_TIME " + json.dumps(out), flush=True)


def run_child(args, config, leg, lib=None):
    env = dict(os.environ)
    if lib:
        env["RAU_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--config", str(config), "--steps",
           str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child {leg} (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("MERGE_TIME "):
            return json.loads(line[len("MERGE_TIME "):])
    raise SystemExit(f"child {leg} printed no result:\n{p.stdout[-2000:]}")


def summary(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "spread_ms": round(float(max(ts) - min(ts)), 4),
            "rounds": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librau.so of the commit before the feature (optional)")
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2], choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--leg", default=None, help="(internal) run one child leg")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    for config in args.configs:
        res = {"tool": "merge_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in LEGS:
            res[leg] = summary(r[leg])
        res["merged_extra_ms"] = round(res["merged"]["median_ms"] - res["null"]["median_ms"], 4)
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            both = res["parent_before"]["rounds"] + res["parent_after"]["rounds"]
            res["parent"] = summary(both)
            d = res["null"]["median_ms"] - res["parent"]["median_ms"]
            res["null_minus_parent_ms"] = round(d, 4)
            res["null_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["profile_merged_step"] = run_child(args, config, "profile")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
