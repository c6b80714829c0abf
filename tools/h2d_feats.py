"""Fresh-batch cost of the training step with f32, 16-bit and fp8 feature maps, on one GPU.

For one workload (configs[1]: Ours_SS B = 256, D = 512, f32; configs[2]: Ours_ResNet B = 256,
D = 2048, bf16 operands) it reports
  * resident_ms          ms/step with the batch resident in HBM (bench.py's metric),
  * step_incl_h2d_ms     ms/step with a fresh batch through the two pinned upload slots every step
                         (batch i+1 uploading while step i runs, as bench.py's H2D leg), per feature type,
  * feat_bytes_per_step  feature bytes one step moves over the link, per feature type,
  * h2d_GBps             achieved pinned host-to-device rate: uploads alone (nothing else on the GPU),
                         feature bytes / wall time of upload + the step stream waiting for it,
  * dropout_features_ms  the train-mode feature-map dropout pass alone (rau_prof class `dropout_features`,
                         serialised by the profiler's events) reading a resident batch of each feature type.
One JSON line per run.  Usage (one workload per process):

    python tools/h2d_feats.py --config 1 [--steps 20] [--feat16 f16|bf16] [--types f32,f16,e4m3]

--types names the feature types measured, in order (default: f32, the --feat16 type, e4m3); a library
older than the fp8 types (RAU_LIB) is measured with --types f32,f16.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {1: dict(name="configs[1]", D=512, dtype="f32", variant="SS"),
             2: dict(name="configs[2]", D=2048, dtype="bf16", variant="ResNet")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--feat16", choices=("f16", "bf16"), default="f16")
    ap.add_argument("--types", default=None, help="comma-separated feature types (default: f32,<feat16>,e4m3)")
    ap.add_argument("--prof-steps", type=int, default=5, help="profiled steps per type for dropout_features_ms")
    args = ap.parse_args()
    types = args.types.split(",") if args.types else ["f32", args.feat16, "e4m3"]
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import feat16, synth
    from rau_vqa_amd.model import RAU, Config, hop_weights

    w = WORKLOADS[args.config]
    cfg = Config(B=256, T=26, V=14000, E=200, Rq=512, D=w["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=w["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    m.training()
    hop_w = hop_weights(w["variant"], cfg.H, 0)
    batches = [synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123 + i, lens="full")
               for i in range(2)]
    n = cfg.B * cfg.D * cfg.S

    def step(i):
        m.set_dropout_seed(123, i)
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def timed(body, count):
        for i in range(args.warmup):
            body(i)
        m.sync()
        t0 = time.perf_counter()
        for i in range(count):
            body(args.warmup + i)
        m.sync()
        return (time.perf_counter() - t0) / count * 1e3

    def fill(ft):
        for sl in (0, 1):
            v = m.batch_slot(sl, feat_type=ft)
            b = batches[sl]
            feat16.store(v["feats"], b["feats"].reshape(v["feats"].shape), ft)
            for k in ("tokens", "lens", "labels"):
                v[k][...] = np.asarray(b[k]).reshape(v[k].shape)

    out = {"workload": w["name"], "B": cfg.B, "D": cfg.D, "S": cfg.S, "dtype": w["dtype"],
           "variant": w["variant"], "steps": args.steps}
    m.set_batch(**batches[0])
    out["resident_ms"] = round(timed(step, args.steps), 3)
    for ft in types:
        fill(ft)
        m.set_batch_async(0, feat_type=ft)

        def fresh(i):
            m.use_batch(i & 1)
            m.set_batch_async((i + 1) & 1, feat_type=ft)   # the next batch uploads under this step
            step(i)
        m.use_batch(0)
        out[f"step_incl_h2d_ms_{ft}"] = round(timed(fresh, args.steps), 3)

        def upload(i):                                   # uploads alone: the link's achieved rate
            m.set_batch_async(i & 1, feat_type=ft)
            m.use_batch(i & 1)
            m.sync()
        ms = timed(upload, args.steps)
        nbytes = n * feat16.dtype_of(ft).itemsize
        out[f"feat_bytes_per_step_{ft}"] = nbytes
        out[f"upload_ms_{ft}"] = round(ms, 3)
        out[f"h2d_GBps_{ft}"] = round(nbytes / ms / 1e6, 2)
    for ft in types:                                     # the dropout pass alone, per input type
        typed = np.empty(batches[0]["feats"].shape, feat16.dtype_of(ft))
        feat16.store(typed, batches[0]["feats"], ft)
        m.set_batch(**dict(batches[0], feats=typed), feat_type=ft)
        step(0)
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        for i in range(args.prof_steps):
            step(1 + i)
        p = m.prof()["dropout_features"]
        m.prof_enable(False)
        out[f"dropout_features_ms_{ft}"] = round(p["ms"] / p["launches"], 4)
        out[f"dropout_features_GBps_{ft}"] = round(p["bytes"] / p["ms"] / 1e6, 1)
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
