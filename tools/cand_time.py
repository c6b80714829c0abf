"""Step time with multiple-choice candidates (rau_set_candidates; cand_head.hip, cand_rank.hip), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident with an answer set of G = 10 entries (tools/bce_time.py's) and,
in the legs that have them, C = 18 candidates per sample (VQA v1's choices: the set's ids plus other answers); a step =
zero_grads + forward + backward + sync at the end of the timed window:
  (a) parent_ms  the step of ANOTHER build of the library given with --parent-lib (the commit before this feature,
                 built by the caller: it is not part of the tree), against
      plain_ms   this build on the batch WITHOUT candidates: launch for launch the parent's step.  The bar is the
                 parent's own run-to-run spread (max - min of its rounds);
  (b) cand_ms    this build with the candidates attached: cand_fwd in ce_set_fwd's place;
  (c) the head launches of one step on their own (cand_fwd against ce_set_fwd), from the library's per-launch events
      (rau_prof_enable);
  (d) stats_ms   rau_topk_cand(k = 3) + rau_cand_stats behind an evaluate-mode forward, against
      host_ms    downloading the [H,n,K] logits (and do_pred, attention) and predict.top_candidates in numpy.
Method: every leg is warmed up, then timed over --steps steps, --rounds times (five by default); the two legs of this
build alternate inside one process, and the parent runs as a child process of its own BEFORE and AFTER them (a library
is loaded once per process), so that drift over the visit shows in the parent's own numbers.  Reported per leg: the
median of the rounds and their spread (max - min).  One JSON line per config:

    python tools/cand_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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

from tools.bce_time import CONFIGS, G, answer_set, summary   # noqa: E402  (the same configs and answer sets)

LEGS = ("plain", "cand")
C_MC = 18
TAG = "CAND_TIME "


def candidates(ids, K, seed=9):
    """C_MC choices per question: the set's ids and other answers, shuffled; cand [B, C_MC] int32"""
    rng = np.random.default_rng(seed)
    cand = np.zeros((ids.shape[0], C_MC), np.int32)
    for b, row in enumerate(ids):
        own = [int(i) for i in row if i > 0]
        others = [int(k) for k in rng.permutation(K) + 1 if k not in own][:C_MC - len(own)]
        cand[b] = rng.permutation(own + others)
    return cand


def child(args):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import predict, synth
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=256, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    batch = synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123, lens="full")
    answers = answer_set(cfg.B, cfg.K)
    cand = candidates(answers[0], cfg.K)
    m.set_batch(**batch, answers=answers)
    m.training()
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    n = [0]

    def attach(leg):
        if leg == "cand":
            m.set_candidates(cand)
        elif leg == "plain":                   # (the parent's library has no such call: its batch never had them)
            m.clear_candidates()

    def step():
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def timed(leg):
        attach(leg)
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
        for leg, name in (("plain", "ce_set_fwd"), ("cand", "cand_fwd")):
            attach(leg)
            for _ in range(args.warmup):
                step()
            m.sync()
            m.prof_enable(True)
            m.prof_reset()
            step()
            m.sync()
            prof = m.prof()
            m.prof_enable(False)
            e = prof.get(name)
            if e and e["launches"]:
                out[name] = {"launches": int(e["launches"]), "ms_per_step": round(float(e["ms"]), 4)}
            m.forward()
            out[leg + "_losses"] = [round(float(v), 4) for v in m.losses()]
    elif args.leg == "stats":
        m.evaluate()
        m.set_candidates(cand)
        m.forward()
        m.sync()
        dev, host = [], []
        for r in range(args.rounds + 1):       # (the first round warms both paths up)
            t0 = time.perf_counter()
            m.top_candidates(3)
            m.cand_stats()
            t1 = time.perf_counter()
            tab_pred, _ = predict.merge_hops(m.logits(), m.dopred(), m.attention())
            predict.top_candidates(tab_pred, cand, 3)
            t2 = time.perf_counter()
            if r:
                dev.append(round((t1 - t0) * 1e3, 4))
                host.append(round((t2 - t1) * 1e3, 4))
        out = {"stats": dev, "host": host}
    else:
        legs = ["parent"] if args.leg == "parent" else list(LEGS)
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
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"child {leg} (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith(TAG):
            return json.loads(line[len(TAG):])
    raise SystemExit(f"child {leg} printed no result:\n{p.stdout[-2000:]}")


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
        res = {"tool": "cand_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8, "G": G,
               "C": C_MC, "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in LEGS:
            res[leg] = summary(r[leg])
        res["cand_minus_plain_ms"] = round(res["cand"]["median_ms"] - res["plain"]["median_ms"], 4)
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            both = res["parent_before"]["rounds"] + res["parent_after"]["rounds"]
            res["parent"] = summary(both)
            d = res["plain"]["median_ms"] - res["parent"]["median_ms"]
            res["plain_minus_parent_ms"] = round(d, 4)
            res["plain_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["profile"] = run_child(args, config, "profile")
        s = run_child(args, config, "stats")
        res["stats"], res["host"] = summary(s["stats"]), summary(s["host"])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
