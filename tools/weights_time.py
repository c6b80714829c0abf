"""Cost of per-sample loss weights (rau_set_sample_weights) in the training step, one GPU.

The kernels that form the training terms gain one 4-byte load per workgroup that owns a row.  Per workload --
configs[1] (Ours_SS, 14x14x512, f32, B = 256) and configs[2] (Ours_ResNet, 14x14x2048, bf16, B = 256), the steps
bench.py times (zero_grads + forward + backward, inputs resident, fresh Philox masks every step) -- the step time in
three states of the batch:
  * none    without weights;
  * ones    with weights all = 1 (the same results bit for bit);
  * random  with weights uniform in [0, 2].
--runs timed runs of --steps steps each per state, interleaved (none, ones, random, none, ...) so that drift of the
box shows in all three alike; every run's ms/step is reported, with min, median and max.  One JSON line per
workload, each measured in a process of its own:

    python tools/weights_time.py [--configs 1 2] [--runs 5] [--steps 20] [--warmup 3]

RAU_LIB=<another build of librau.so> measures that build; one without rau_set_sample_weights (the parent commit's,
for its run-to-run spread on the same box on the same day: measure it before and after this build) reports the
state `none` only.
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

CONFIGS = {1: dict(D=512, dtype="f32", variant="SS"), 2: dict(D=2048, dtype="bf16", variant="ResNet")}


def one(which, runs, steps, warmup):
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import synth
    from rau_vqa_amd.model import RAU, Config, hop_weights
    w = CONFIGS[which]
    cfg = Config(B=256, T=26, V=14000, E=200, Rq=512, D=w["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=w["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    batch = synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123, lens="full")
    hop_w = hop_weights(w["variant"], cfg.H, 0)
    m.training()
    rng = np.random.default_rng(7)
    states = {"none": None}
    if hasattr(m._lib, "rau_set_sample_weights"):
        states["ones"] = np.ones(cfg.B, np.float32)
        states["random"] = rng.uniform(0, 2, cfg.B).astype(np.float32)
    it = [0]

    def run(n):
        for _ in range(n):
            m.set_dropout_seed(123, it[0])
            it[0] += 1
            m.zero_grads()
            m.forward()
            m.backward(hop_w)
        m.sync()
    ms = {k: [] for k in states}
    for _ in range(runs):
        for name, s in states.items():
            m.set_batch(**batch)                       # an upload clears the weights
            if s is not None:
                m.set_sample_weights(s)
            run(warmup)
            t0 = time.perf_counter()
            run(steps)
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    assert np.all(np.isfinite(m.losses()))
    m.close()
    res = {"tool": "weights_time", "config": which, "B": cfg.B, "D": cfg.D, "dtype": w["dtype"], "runs": runs,
           "steps": steps, "warmup": warmup, "lib": os.environ.get("RAU_LIB", "librau.so")}
    for name, v in ms.items():
        res[name + "_ms"] = [round(x, 4) for x in v]
        res[name + "_min_med_max"] = [round(float(f(v)), 4) for f in (np.min, np.median, np.max)]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2], choices=sorted(CONFIGS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", type=int, default=0, help="(internal) measure this workload in this process")
    args = ap.parse_args()
    if args.one:
        one(args.one, args.runs, args.steps, args.warmup)
        return
    for c in args.configs:   # a fresh process per workload: a second context in one process shares its queues
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--one", str(c), "--runs", str(args.runs),
                               "--steps", str(args.steps), "--warmup", str(args.warmup)], cwd=ROOT)


if __name__ == "__main__":
    main()
