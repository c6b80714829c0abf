"""Cost of attention supervision in the step-level backward (rau_backward_att), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the
end of the timed window:
  * parent_ms        the step of ANOTHER build of the library given with --parent-lib (the commit before this
                     feature, built by the caller: it is not part of the tree), through rau_backward;
  * null_ms          this build, rau_backward_att with att_w = NULL, a batch without targets;
  * null_targets_ms  the same call on a batch WITH targets (rau_set_att_targets);
  * att_ms           targets set and att_w = 1 on every hop: the supervised step.
Method: every leg is warmed up, then timed over --steps steps, --rounds times (five by default); the three legs
of this build alternate inside one process, and the parent runs as a child process of its own BEFORE and AFTER
them (a library is loaded once per process), so that drift over the visit shows in the parent's own numbers.
Reported per leg: the median of the rounds and their spread (max - min).  The condition on the two NULL legs:
|leg - parent| within the parent's own spread.  A last child profiles one supervised step per config with the
library's per-launch events (rau_prof_enable) and prints the launch the feature adds (att_sup_grad) beside the
attention backward that reads its output.
One JSON line per config:

    python tools/att_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
LEGS = ("null", "null_targets", "att")


def target_maps(B, S, seed=5):
    """Normalised smooth maps for three rows in four, zeros for the fourth (most questions have no human map)."""
    rng = np.random.default_rng(seed)
    pos = np.arange(S)[None, :]
    t = np.exp(-0.5 * ((pos - rng.uniform(0, S, (B, 1))) / rng.uniform(S / 8, S / 3, (B, 1))) ** 2)
    t /= t.sum(axis=1, keepdims=True)
    t[3::4] = 0
    return np.ascontiguousarray(t, np.float32)


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
    ones = np.ones(cfg.H, np.float32)
    t = target_maps(cfg.B, cfg.S)
    n = [0]
    has = [False]

    def step(leg):
        want = leg in ("null_targets", "att")
        if want != has[0]:                     # outside the timed window: timed() warms up first
            m.set_batch(**batch)
            if want:
                m.set_att_targets(t)
            has[0] = want
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        if leg == "parent":
            m.backward(hop_w)
        elif leg == "att":
            m.backward(hop_w, att_w=ones)
        else:
            check(m._lib.rau_backward_att(m._h, hop_w.ctypes.data, None, None))

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
            step("att")
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        step("att")
        m.sync()
        prof = m.prof()
        m.prof_enable(False)
        for name in ("att_sup_grad", "att_bwd_fused", "att_bwd_split", "head_dgrad", "scale_hops"):
            e = prof.get(name)
            if e and e["launches"]:
                out[name] = {"launches": int(e["launches"]), "ms_per_step": round(float(e["ms"]), 4)}
        m.forward()
        st = m.att_stats()
        out["att_stats"] = {"loss_hop0": round(float(st["loss"][0]), 4), "n_sup": st["n_sup"]}
    else:
        legs = ["parent"] if args.leg == "parent" else list(LEGS)
        out = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print("ATT_TIME " + json.dumps(out), flush=True)


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
        if line.startswith("ATT_TIME "):
            return json.loads(line[len("ATT_TIME "):])
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
        res = {"tool": "att_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in LEGS:
            res[leg] = summary(r[leg])
        res["att_extra_ms"] = round(res["att"]["median_ms"] - res["null_targets"]["median_ms"], 4)
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            both = res["parent_before"]["rounds"] + res["parent_after"]["rounds"]
            res["parent"] = summary(both)
            for leg in ("null", "null_targets"):
                d = res[leg]["median_ms"] - res["parent"]["median_ms"]
                res[leg + "_minus_parent_ms"] = round(d, 4)
                res[leg + "_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["profile_att_step"] = run_child(args, config, "profile")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
