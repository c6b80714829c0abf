"""Step time with the per-position L2 normalisation of the feature maps on the device (rau_set_feat_norm), one GPU.

At bench.py's configs[1] (Ours_SS, B = 256, D = 512, f32) and configs[2] (Ours_ResNet, B = 256, D = 2048, bf16),
training mode, device-drawn masks, the batch resident, a step = zero_grads + forward + backward + sync at the end
of the timed window:
  * parent_ms    the step of ANOTHER build of the library given with --parent-lib (the commit before this feature,
                 built by the caller: it is not part of the tree), run BEFORE and AFTER the legs of this build;
  * off_ms       this build with the switch off (the default): launch for launch the parent's step.  The condition:
                 |off - parent| within the parent's own run-to-run spread;
  * on_f32_ms    the switch on, float32 maps resident;
  * on_e4m3_ms   the switch on, the same maps stored as fp8 e4m3 (widened exactly, normalised in f32);
  * host_ms      for context only: the switch off and the HOST normalising the same float32 batch in numpy inside the
                 loop (one pass in float32 + the upload of the result), timed over --host-steps steps.
Method: every leg is warmed up, then timed over --steps steps, --rounds times (five by default); the legs of this
build alternate inside one process on one context; the parent runs as a child process of its own (a library is
loaded once per process).  Reported per leg: the median of the rounds and their spread (max - min).
A last child profiles one step per stored type with the library's per-launch events (rau_prof_enable), the
feature-map gradient on, and prints the two launches alone: l2norm_features (algorithmic traffic: one read at the
stored width + one float32 write) and l2norm_backward (two float32 reads + one write), with the bytes per second
they reach.  One JSON line per config:

    python tools/featnorm_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
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
LEGS = ("off", "on_f32", "on_e4m3")
EPS = 1e-12


def child(args):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import feat16, synth
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=256, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    batch = synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123, lens="full")
    feats = np.ascontiguousarray(batch["feats"], np.float32)
    m.training()
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    n = [0]

    stored = {}   # the resident maps narrowed to a type, once

    def put(ft="f32", x=None):
        if x is None and ft != "f32" and ft not in stored:
            stored[ft] = np.empty(feats.shape, feat16.dtype_of(ft))
            feat16.store(stored[ft], feats, ft)
        x = x if x is not None else feats if ft == "f32" else stored[ft]
        m.set_batch(x, batch["tokens"], batch["lens"], batch["labels"], feat_type=ft)

    def step():
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def host_step():
        x = feats
        nrm = np.sqrt(np.einsum("nds,nds->ns", x, x))
        put(x=x / np.maximum(nrm, np.float32(EPS))[:, None, :])
        step()

    def timed(leg):
        one, steps = (host_step, args.host_steps) if leg == "host" else (step, args.steps)
        if leg != "parent":   # (the parent's library has no switch)
            m.normalize_features(leg.startswith("on"), EPS)
        put("e4m3" if leg == "on_e4m3" else "f32")
        for _ in range(1 if leg == "host" else args.warmup):
            one()
        m.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        m.sync()
        return (time.perf_counter() - t0) / steps * 1e3

    out = {}
    if args.leg == "profile":
        m.want_feature_grad()
        m.normalize_features(True, EPS)
        elems = float(cfg.B) * cfg.D * cfg.S
        for ft, width in (("f32", 4), ("e4m3", 1)):
            put(ft)
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
            for name, by in (("l2norm_features", elems * (width + 4)), ("l2norm_backward", elems * 12)):
                e = prof[name]
                rec[name] = {"launches": int(e["launches"]), "ms": round(float(e["ms"]), 4),
                             "algorithmic_GB": round(by / 1e9, 4),
                             "TB_per_s": round(by / (float(e["ms"]) * 1e-3) / 1e12, 3)}
            out[ft] = rec
    else:
        legs = ["parent"] if args.leg == "parent" else list(LEGS) + ["host"]
        out = {leg: [] for leg in legs}
        for _ in range(args.rounds):
            for leg in legs:
                out[leg].append(round(timed(leg), 4))
    m.close()
    print("FEATNORM_TIME " + json.dumps(out), flush=True)


def run_child(args, config, leg, lib=None):
    env = dict(os.environ)
    if lib:
        env["RAU_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--config", str(config), "--steps",
           str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--host-steps",
           str(args.host_steps)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=420)
    if p.returncode != 0:
        raise SystemExit(f"child {leg} (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("FEATNORM_TIME "):
            return json.loads(line[len("FEATNORM_TIME "):])
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
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--leg", default=None, help="(internal) run one child leg")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    for config in args.configs:
        res = {"tool": "featnorm_time", "config": f"configs[{config}]", **CONFIGS[config], "B": 256, "H": 8,
               "steps": args.steps}
        if args.parent_lib:
            res["parent_before"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
        r = run_child(args, config, "this")
        for leg in LEGS + ("host",):
            res[leg] = summary(r[leg])
        for leg in LEGS[1:]:
            res[leg + "_minus_off_ms"] = round(res[leg]["median_ms"] - res["off"]["median_ms"], 4)
        if args.parent_lib:
            res["parent_after"] = summary(run_child(args, config, "parent", args.parent_lib)["parent"])
            both = res["parent_before"]["rounds"] + res["parent_after"]["rounds"]
            res["parent"] = summary(both)
            d = res["off"]["median_ms"] - res["parent"]["median_ms"]
            res["off_minus_parent_ms"] = round(d, 4)
            res["off_inside_parent_spread"] = bool(abs(d) <= res["parent"]["spread_ms"])
        res["kernels_in_one_step"] = run_child(args, config, "profile")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
