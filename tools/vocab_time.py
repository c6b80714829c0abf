"""What an answer count that is no multiple of four costs (rau_logits_pitch), one GPU.

At bench.py's configs[1] (Ours_SS, D = 512, f32) and configs[2] (Ours_ResNet, D = 2048, bf16) with B = 256 and
H = 8, device-drawn masks, the batch resident, two legs:
  * train   zero_grads + forward + backward;
  * eval    the evaluate-mode forward alone (the inference leg).
Vocabularies: K = 3128, 3129 and 3132 on this build, and K = 3128 and 3132 on ANOTHER build of the library given
with --parent-lib (the commit before this feature, built by the caller: it is not part of the tree, and it refuses
3129).  K = 1000 is bench.py's headline shape, timed on both builds as a control.  The comparison that matters:
K = 3129 here against K = 3132 on the parent -- the padding workaround this feature replaces.  With the pitch the two
run the same kernel classes on the same tiles, so the expectation is equality within the parent's own spread.

Method: a window is bracketed by two device events on the context's stream, the second one recorded behind a drain
of all of the context's streams; every leg is warmed up, then timed over --steps steps, --rounds times (five by
default), the two legs alternating inside one child process per (build, K); the parent's children run BEFORE and
AFTER this build's, so that drift over the visit shows in the parent's own numbers.  Reported per leg: the median of
the rounds and their spread (max - min).  A last pair of children profiles one train step at K = 3129 and 3132 with
the library's per-launch events (rau_prof_enable) and prints the classes the answer count shapes: the head's GEMMs,
its criterion kernel (whose pad writes are the feature's only extra stores) and the classifier's gradients.
One JSON line per config:

    python tools/vocab_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {1: dict(D=512, dtype="f32"), 2: dict(D=2048, dtype="bf16")}   # bench.py: configs[1], configs[2]
LEGS = ("train", "eval")
KS_THIS = (1000, 3128, 3129, 3132)
KS_PARENT = (1000, 3128, 3132)
HEAD_CLASSES = ("head_gemm", "ce_fwd", "ce_set_fwd", "bce_fwd", "scale_hops", "head_dgrad", "mult_wgrad",
                "wgrad_group", "loss_reduce")


def child(args):
    import torch  # (before librau.so: one HIP runtime)
    from rau_vqa_amd import synth
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=256, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=args.K, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    batch = synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123, lens="full")
    m.set_batch(**batch)
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    own = torch.cuda.ExternalStream(m.stream(), device=torch.device("cuda", cfg.device_id))
    n = [0]

    def step(leg):
        if leg == "eval":
            m.forward()
            return
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def timed(leg):
        m.training() if leg == "train" else m.evaluate()
        for _ in range(args.warmup):
            step(leg)
        m.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(own)
        for _ in range(args.steps):
            step(leg)
        m.sync()            # every stream of the context has drained: the window ends here
        e1.record(own)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    out = {}
    if args.leg == "profile":
        m.training()
        for _ in range(args.warmup):
            step("train")
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        step("train")
        m.sync()
        prof = m.prof()
        m.prof_enable(False)
        for name, e in sorted(prof.items()):
            if e["launches"] and (name in HEAD_CLASSES or "wgrad" in name or name.startswith("head")):
                out[name] = {"launches": int(e["launches"]), "ms": round(float(e["ms"]), 4)}
    else:
        out = {leg: [] for leg in LEGS}
        for _ in range(args.rounds):
            for leg in LEGS:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print("VOCAB_TIME " + json.dumps(out), flush=True)


def run_child(args, config, K, leg, lib=None):
    env = dict(os.environ)
    if lib:
        env["RAU_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--config", str(config), "--K", str(K),
           "--steps", str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child {leg} K={K} (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("VOCAB_TIME "):
            return json.loads(line[len("VOCAB_TIME "):])
    raise SystemExit(f"child {leg} K={K} printed no result:\n{p.stdout[-2000:]}")


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
    ap.add_argument("--leg", default=None, help="(internal) run one child")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    ap.add_argument("--K", type=int, default=1000, help="(internal)")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    for config in args.configs:
        res = {"tool": "vocab_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        parent = {K: {leg: [] for leg in LEGS} for K in KS_PARENT}
        if args.parent_lib:
            for K in KS_PARENT:
                r = run_child(args, config, K, "time", args.parent_lib)
                for leg in LEGS:
                    parent[K][leg] += r[leg]
        this = {K: run_child(args, config, K, "time") for K in KS_THIS}
        if args.parent_lib:
            for K in KS_PARENT:
                r = run_child(args, config, K, "time", args.parent_lib)
                for leg in LEGS:
                    parent[K][leg] += r[leg]
        for leg in LEGS:
            res[leg] = {"this": {str(K): summary(this[K][leg]) for K in KS_THIS}}
            if args.parent_lib:
                res[leg]["parent"] = {str(K): summary(parent[K][leg]) for K in KS_PARENT}
                p, t = res[leg]["parent"], res[leg]["this"]
                for name, kt, kp in (("k3129_minus_parent_k3132", "3129", "3132"),
                                     ("k3132_minus_parent_k3132", "3132", "3132"),
                                     ("k1000_minus_parent_k1000", "1000", "1000")):
                    d = t[kt]["median_ms"] - p[kp]["median_ms"]
                    res[leg][name] = {"ms": round(d, 4), "inside_parent_spread": bool(abs(d) <= p[kp]["spread_ms"])}
        res["profile_train_step"] = {str(K): run_child(args, config, K, "profile") for K in (3129, 3132)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
