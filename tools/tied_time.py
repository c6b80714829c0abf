"""Step time with the feature-map dropout mask tied across the hops (rau_set_feat_dropout, RAU_XDROP_TIED)
against the reference's mask per hop clone, one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the
end of the timed window:
  * parent_ms    the per-hop step of ANOTHER build of the library given with --parent-lib (the commit before this
                 feature, built by the caller: it is not part of the tree);
  * per_hop_ms   this build with the switch off (the default): launch for launch the parent's step;
  * tied_ms      this build with the switch on: one masked map, both convs once, the hops summed in front of one
                 set of conv gradients.
Method: every leg is warmed up, then timed over --steps steps, --rounds times (five by default); the two legs of
this build alternate inside one process on one context (the switch is flipped between them), and the parent runs
as a child process of its own BEFORE and AFTER them (a library is loaded once per process), so that drift over
the visit shows in the parent's own numbers.  Reported per leg: the median of the rounds and their spread
(max - min).  The condition on the per-hop leg: |per_hop - parent| within the parent's own spread.  A last child
profiles one step of either kind per config with the library's per-launch events (rau_prof_enable: launches are
bracketed, so streams overlap less than in the timed legs) and prints the five conv classes, the two launches the
tied backward adds (hop_sum, outer_sum) and the feature-map dropout pass, with the sum over each stream's classes:
where tied is not faster than per-hop, the stream whose sum is the largest is what bounds the step.
One JSON line per config:

    python tools/tied_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
LEGS = ("per_hop", "tied")
CONV_CLASSES = ("conv_embed_fwd", "conv_att_pre", "conv_att_dgrad", "conv_att_wgrad", "conv_embed_wgrad")
BULK_CLASSES = CONV_CLASSES + ("hop_sum", "outer_sum", "dropout_features", "transpose", "colsum")
# the recurrence's stream: what a step is left with once the convs are off its critical path
CHAIN_CLASSES = ("embed_fwd", "enc_i2h_gemm", "enc_h2h_gemm", "enc_ws", "lstm_fwd", "gather_q", "apply_mask",
                 "q_proj_gemm", "small_gemm", "lin_reduce", "att_fwd_fused", "att_fwd_fused_regs", "att_fwd_split",
                 "loss_reduce", "scale_hops", "head_dgrad", "lstm_bwd", "att_bwd_fused", "att_bwd_split",
                 "q_proj_dgrad", "dq_reduce", "enc_h2h_dgrad", "enc_i2h_dgrad", "embed_bwd")


def child(args):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import synth
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
    n = [0]

    def step():
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def timed(leg):
        if leg != "parent":   # (the parent's library has no switch)
            m.tie_feature_dropout(leg == "tied")
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
        for leg in LEGS:
            m.tie_feature_dropout(leg == "tied")
            for _ in range(args.warmup):
                step()
            m.sync()
            m.prof_enable(True)
            m.prof_reset()
            step()
            m.sync()
            prof = m.prof()
            m.prof_enable(False)
            rec = {}
            for name in CONV_CLASSES + ("hop_sum", "outer_sum", "dropout_features"):
                e = prof.get(name)
                if e and e["launches"]:
                    rec[name] = {"launches": int(e["launches"]), "ms": round(float(e["ms"]), 4)}
            rec["bulk_stream_classes_ms"] = round(sum(prof[k]["ms"] for k in BULK_CLASSES if k in prof), 4)
            rec["chain_stream_classes_ms"] = round(sum(prof[k]["ms"] for k in CHAIN_CLASSES if k in prof), 4)
            out[leg] = rec
    else:
        legs = ["parent"] if args.leg == "parent" else list(LEGS)
        out = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print("TIED_TIME " + json.dumps(out), flush=True)


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
        if line.startswith("TIED_TIME "):
            return json.loads(line[len("TIED_TIME "):])
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
        res = {"tool": "tied_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in LEGS:
            res[leg] = summary(r[leg])
        res["tied_minus_per_hop_ms"] = round(res["tied"]["median_ms"] - res["per_hop"]["median_ms"], 4)
        res["tied_faster"] = bool(res["tied_minus_per_hop_ms"] < 0)
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            both = res["parent_before"]["rounds"] + res["parent_after"]["rounds"]
            res["parent"] = summary(both)
            d = res["per_hop"]["median_ms"] - res["parent"]["median_ms"]
            res["per_hop_minus_parent_ms"] = round(d, 4)
            res["per_hop_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["profile_one_step"] = run_child(args, config, "profile")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
