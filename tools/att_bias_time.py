"""Step time with an attention bias attached (rau_set_att_bias_dev), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the end
of the timed window:
  * nobias_ms       the step without a bias (its launches are the parent's, its attention kernels test one null
                    pointer per workgroup: it must sit inside the parent's own run-to-run spread);
  * bias_ms         the step with a bias [n,S] attached: every hop's attention kernel reads a row of it and
                    att_bias_grad follows the hop loop.  The bias (2 * standard normal, every fourth position of
                    every second row at -inf) is attached once, outside the timed window;
  * parent_ms       the no-bias step of ANOTHER build of the library given with --parent-lib (the commit before this
                    feature, built by the caller: it is not part of the tree).
Method: every leg is warmed up, then timed over --steps steps, --rounds times; the legs of this build alternate inside
one process, and the parent library runs as a child process of its own BEFORE and AFTER this build's.  Reported per
leg: the median of the rounds and their spread (max - min).  One JSON line per config:

    python tools/att_bias_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
TAG = "ATT_BIAS_TIME "
LEGS = ("nobias", "bias")


def child(args):
    import torch
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
    n = [0]
    st = {"leg": None, "bias": None}

    def step():
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def enter(leg):
        if st["leg"] == leg:
            return
        if leg == "bias":
            if st["bias"] is None:
                g = torch.Generator(device="cuda").manual_seed(1)
                b = 2 * torch.randn(cfg.B, cfg.S, device="cuda", generator=g)
                b[::2, ::4] = float("-inf")
                torch.cuda.synchronize()
                st["bias"] = b
            m.set_att_bias(st["bias"])
        else:
            m.clear_att_bias()
        st["leg"] = leg

    def timed(leg):
        if leg != "parent":              # an older build: nothing of the new interface is called
            enter(leg)
        for _ in range(args.warmup):
            step()
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        m.sync()
        return (time.perf_counter() - t0) / args.steps * 1e3

    legs = ("parent",) if args.leg == "parent" else LEGS
    out = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            out[leg].append(round(timed(leg), 4))
    m.close()
    print(TAG + json.dumps(out), flush=True)


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
        if line.startswith(TAG):
            return json.loads(line[len(TAG):])
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
        res = {"tool": "att_bias_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in LEGS:
            res[leg] = summary(r[leg])
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            res["parent"] = summary(res["parent_before"]["rounds"] + res["parent_after"]["rounds"])
            d = res["nobias"]["median_ms"] - res["parent"]["median_ms"]
            res["nobias_minus_parent_ms"] = round(d, 4)
            res["nobias_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["bias_minus_nobias_ms"] = round(res["bias"]["median_ms"] - res["nobias"]["median_ms"], 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
