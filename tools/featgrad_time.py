"""Cost of the feature-map gradient in the step-level backward (rau_set_feat_grad), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the end
of the timed window:
  * off_ms      the step with the switch off (it must sit inside the parent's own run-to-run spread);
  * on_ms       the switch on, the default dispatch: per hop a GEMM into a one-hop temporary + a masked accumulate;
  * fused_ms    the switch on under RAU_XGRAD_FUSED=1 (the fused kernel where it applies: f32, 14 x 14 class; in
                bf16 mode there is no fused tile and the leg repeats the default), a child process of its own;
  * tied_ms     the switch on under the tied feature-map dropout (one mask: one product at n = B);
  * parent_ms   the step of ANOTHER build of the library given with --parent-lib (the commit before this feature,
                built by the caller: it is not part of the tree).
Method: every leg is warmed up, then timed over --steps steps, --rounds times; off / on / tied alternate inside one
process, started with RAU_XGRAD_FUSED=0; the fused leg runs in a child started with RAU_XGRAD_FUSED=1 (a context
reads the variable when it is created; a process per setting keeps the legs apart) and the parent library runs as a
child process of its own BEFORE and AFTER this build's.  Reported per leg: the median of the rounds and their spread
(max - min); fused_gain_ms = on - fused, and fused_beats_default says whether that exceeds the larger of the two
spreads.  A last pair of children profiles one step with the switch on (profile_on: the default, profile_fused:
RAU_XGRAD_FUSED=1) with the library's per-launch events and prints the conv_embed_dgrad / xgrad_accum / mul_dtanh
launches: time per step and, from the class's FLOP count, the fraction of the 157.3 TF f32 matrix peak.
One JSON line per config:

    python tools/featgrad_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
TAG = "FEATGRAD_TIME "
PEAK_F32_MATRIX = 157.3e12


def child(args):
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
    state = {"leg": None}

    def enter(leg):
        if state["leg"] == leg:
            return
        state["leg"] = leg
        if leg == "parent":
            return
        m.tie_feature_dropout(leg == "tied")
        m.want_feature_grad(leg != "off")

    def step():
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def timed(leg):
        enter(leg)
        for _ in range(args.warmup):
            step()
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        m.sync()
        return (time.perf_counter() - t0) / args.steps * 1e3

    out = {}
    if args.leg == "profile":
        enter("on")
        for _ in range(args.warmup):
            step()
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        step()
        m.sync()
        prof = m.prof()
        m.prof_enable(False)
        for name in ("conv_embed_dgrad", "xgrad_accum", "mul_dtanh", "conv_att_dgrad", "conv_embed_wgrad"):
            e = prof.get(name)
            if e:
                ms = float(e["ms"])
                out[name] = {"launches": int(e["launches"]), "ms_per_step": round(ms, 4)}
                if e.get("flops") and ms > 0:
                    out[name]["of_f32_matrix_peak"] = round(float(e["flops"]) / (ms * 1e-3) / PEAK_F32_MATRIX, 3)
    else:
        legs = {"parent": ["parent"], "this": ["off", "on", "tied"], "fused": ["on"]}[args.leg]
        out = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print(TAG + json.dumps(out), flush=True)


def run_child(args, config, leg, lib=None, env_extra=None):
    env = dict(os.environ)
    if lib:
        env["RAU_LIB"] = os.path.abspath(lib)
    env.update(env_extra or {})
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
    default, fused = {"RAU_XGRAD_FUSED": "0"}, {"RAU_XGRAD_FUSED": "1"}
    for config in args.configs:
        res = {"tool": "featgrad_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this", env_extra=default)
        for leg in ("off", "on", "tied"):
            res[leg] = summary(r[leg])
        res["fused"] = summary(run_child(args, config, "fused", env_extra=fused)["on"])
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            res["parent"] = summary(res["parent_before"]["rounds"] + res["parent_after"]["rounds"])
            d = res["off"]["median_ms"] - res["parent"]["median_ms"]
            res["off_minus_parent_ms"] = round(d, 4)
            res["off_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["on_minus_off_ms"] = round(res["on"]["median_ms"] - res["off"]["median_ms"], 4)
        res["fused_minus_off_ms"] = round(res["fused"]["median_ms"] - res["off"]["median_ms"], 4)
        gain = res["on"]["median_ms"] - res["fused"]["median_ms"]
        res["fused_gain_ms"] = round(gain, 4)
        res["fused_beats_default"] = bool(gain > max(res["on"]["spread_ms"], res["fused"]["spread_ms"]))
        res["profile_on"] = run_child(args, config, "profile", env_extra=default)
        res["profile_fused"] = run_child(args, config, "profile", env_extra=fused)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
