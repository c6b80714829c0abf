"""Cost of the step-level backward from caller-supplied gradients (rau_backward_ext), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the
end of the timed window:
  * plain_ms     the step through rau_backward (this path is unchanged: it must sit inside the parent's spread);
  * select_ms    the step through rau_backward_select with select_w = 1 on every hop -- the fair baseline: it also
                 forms dpre / dhn in the backward;
  * ext_ms       the step through rau_backward_ext with all three gradients resident in device memory (fixed
                 tensors of the size of a CE gradient; what the caller spends on computing them is not part of it);
  * parent_ms    the step of ANOTHER build of the library given with --parent-lib (the commit before this feature,
                 built by the caller: it is not part of the tree), through rau_backward.
Method: every leg is warmed up, then timed over --steps steps, --rounds times; legs alternate inside one process
(plain, select, ext, plain, ...) and the parent library runs as a child process of its own BEFORE and AFTER this
build's (a library is loaded once per process).  Reported per leg: the median of the rounds and their spread
(max - min).  A last child profiles one ext step per config with the library's per-launch events
(rau_prof_enable) and prints the three launches the feature adds -- ext_dl, ext_signal, ext_da -- and the classes
around them (head_dgrad, select_wgrad, scale_hops).
One JSON line per config:

    python tools/ext_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
TAG = "EXT_TIME "


def child(args):
    import torch  # (before librau.so: one HIP runtime)
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
    grads = None
    if args.leg != "parent":
        gen = torch.Generator(device="cuda").manual_seed(5)
        rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen) / cfg.B
        grads = {"logits": rnd(cfg.H, cfg.B, cfg.K), "dopred": rnd(cfg.H, cfg.B), "attprob": rnd(cfg.H, cfg.B, cfg.S)}
        torch.cuda.synchronize()
    n = [0]

    def step(leg):
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        if leg in ("parent", "plain"):
            m.backward(hop_w)
        elif leg == "select":
            m.backward(hop_w, ones)
        else:
            m.backward(hop_w, out_grads=grads)

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
            step("ext")
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        step("ext")
        m.sync()
        prof = m.prof()
        m.prof_enable(False)
        for name in ("ext_dl", "ext_signal", "ext_da", "head_dgrad", "select_wgrad", "scale_hops"):
            e = prof.get(name)
            if e:
                out[name] = {"launches": int(e["launches"]), "ms_per_step": round(float(e["ms"]), 4)}
    else:
        legs = ["parent"] if args.leg == "parent" else ["plain", "select", "ext"]
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
        res = {"tool": "ext_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in ("plain", "select", "ext"):
            res[leg] = summary(r[leg])
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            both = res["parent_before"]["rounds"] + res["parent_after"]["rounds"]
            res["parent"] = summary(both)
            d = res["plain"]["median_ms"] - res["parent"]["median_ms"]
            res["plain_minus_parent_ms"] = round(d, 4)
            res["plain_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["ext_minus_select_ms"] = round(res["ext"]["median_ms"] - res["select"]["median_ms"], 4)
        res["ext_minus_plain_ms"] = round(res["ext"]["median_ms"] - res["plain"]["median_ms"], 4)
        res["profile_ext_step"] = run_child(args, config, "profile")
        res["ext_launches_ms"] = round(sum(res["profile_ext_step"].get(k, {}).get("ms_per_step", 0.0)
                                           for k in ("ext_dl", "ext_signal", "ext_da")), 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
