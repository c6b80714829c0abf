"""Step time under the sigmoid answer head (rau_set_answer_loss, RAU_LOSS_BCE; bce_head.hip), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident with an answer set of G = 10 entries (ten human answers,
weights min(count / 3, 1)), a step = zero_grads + forward + backward + sync at the end of the timed window:
  * parent_ms   the step of ANOTHER build of the library given with --parent-lib (the commit before this
                feature, built by the caller: it is not part of the tree): the softmax criterion against the set;
  * ce_ms       this build, the softmax criterion (ce_set_fwd): launch for launch the parent's step;
  * bce_ms      this build after rau_set_answer_loss(RAU_LOSS_BCE): bce_fwd in ce_set_fwd's place.
Method: every leg is warmed up, then timed over --steps steps, --rounds times (five by default); the two legs of
this build alternate inside one process, and the parent runs as a child process of its own BEFORE and AFTER them
(a library is loaded once per process), so that drift over the visit shows in the parent's own numbers.  Reported
per leg: the median of the rounds and their spread (max - min).  The expectation: |bce - parent| and |ce - parent|
within the parent's own spread -- the head does the same passes over [H B, K] under either criterion.  A last child
profiles one step of each kind with the library's per-launch events (rau_prof_enable) and prints the head launch
(bce_fwd, ce_set_fwd) on its own.
One JSON line per config:

    python tools/bce_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
LEGS = ("ce", "bce")
G = 10


def answer_set(B, K, seed=7):
    """Ten human answers per question over two to four distinct ids: ids [B, G] (0 = empty), w = min(count / 3, 1)"""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, G), np.int32)
    w = np.zeros((B, G), np.float32)
    for b in range(B):
        n = int(rng.integers(2, 5))
        picks = rng.choice(K, size=n, replace=False) + 1
        counts = rng.multinomial(10, np.full(n, 1.0 / n))
        ids[b, :n] = picks
        w[b, :n] = np.minimum(counts / 3.0, 1.0)
    return ids, w


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
    m.set_batch(**batch, answers=answer_set(cfg.B, cfg.K))
    m.training()
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    n = [0]

    def step(leg):
        if leg != "parent":                    # (the parent's library has no switch)
            m.set_answer_loss(leg)
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

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
        for leg, name in (("ce", "ce_set_fwd"), ("bce", "bce_fwd")):
            for _ in range(args.warmup):
                step(leg)
            m.sync()
            m.prof_enable(True)
            m.prof_reset()
            step(leg)
            m.sync()
            prof = m.prof()
            m.prof_enable(False)
            e = prof.get(name)
            if e and e["launches"]:
                out[name] = {"launches": int(e["launches"]), "ms_per_step": round(float(e["ms"]), 4)}
            m.forward()
            out[leg + "_losses"] = [round(float(v), 4) for v in m.losses()]
    else:
        legs = ["parent"] if args.leg == "parent" else list(LEGS)
        out = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print("BCE_TIME " + json.dumps(out), flush=True)


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
        if line.startswith("BCE_TIME "):
            return json.loads(line[len("BCE_TIME "):])
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
        res = {"tool": "bce_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8, "G": G,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in LEGS:
            res[leg] = summary(r[leg])
        res["bce_minus_ce_ms"] = round(res["bce"]["median_ms"] - res["ce"]["median_ms"], 4)
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            both = res["parent_before"]["rounds"] + res["parent_after"]["rounds"]
            res["parent"] = summary(both)
            for leg in LEGS:
                d = res[leg]["median_ms"] - res["parent"]["median_ms"]
                res[f"{leg}_minus_parent_ms"] = round(d, 4)
                res[f"{leg}_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["profile"] = run_child(args, config, "profile")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
