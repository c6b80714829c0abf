"""Fresh-batch cost of the training step with region features: dense maps against packed rows, on one GPU.

Workload: B = 256 images of 10..100 boxes (uniform, seeded) at S = 100, D = 2048, bf16 mode, f32 features (or
--feat-type), a fresh batch every step through the two pinned upload slots (batch i+1 uploading while step i runs).
Legs, ms/step:
  a  dense_ms         dense [B, D, S] batches prepared outside the timed loop (staging filled once) + set_regions;
  b  dense_host_ms    dense batches, the host transposing and zero-padding every image's rows into the staging inside
                      the loop: what a user of region files does without the packed entry points;
  c  packed_ms        packed rows prepared outside the timed loop (rows at the start of the staging, filled once);
  d  packed_host_ms   packed rows copied (concatenated, no transpose, no padding) into the staging inside the loop.
Also: the link bytes per step of both forms, the uploads alone (nothing else on the GPU), and the unpack launch alone
(rau_prof class `unpack_regions`, serialised by the profiler's events).  One JSON line per run.  Usage:

    python tools/packed_time.py [--steps 20] [--legs a,b,c,d] [--feat-type f32|f16|bf16|e4m3]

Legs a and b run code that exists without the packed entry points: a library older than them (RAU_LIB) is measured
with --legs a,b.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--feat-type", default="f32")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--prof-steps", type=int, default=5)
    args = ap.parse_args()
    legs = args.legs.split(",")
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import feat16
    from rau_vqa_amd.model import RAU, Config, hop_weights

    ft = feat16.check_name(args.feat_type)
    cfg = Config(B=args.batch, T=26, V=14000, E=200, Rq=512, D=2048, S=100, M=512, A=256, R=512, K=1000, H=8,
                 dtype="bf16")
    B, D, S = cfg.B, cfg.D, cfg.S
    m = RAU(cfg)
    m.init_uniform(seed=123)
    m.training()
    hop_w = hop_weights("ResNet", cfg.H, 0)
    rng = np.random.default_rng(123)
    data = []                                            # two batches: rows, counts, offsets, the question side
    for _ in range(2):
        counts = rng.integers(10, S + 1, B).astype(np.int32)
        rows = np.empty((int(counts.sum()), D), feat16.dtype_of(ft))
        feat16.store(rows, rng.standard_normal(rows.shape, np.float32), ft)
        tokens = rng.integers(2, cfg.V + 1, (cfg.T, B)).astype(np.int32)
        data.append(dict(rows=rows, counts=counts, off=np.concatenate([[0], np.cumsum(counts)[:-1]]),
                         tokens=tokens, lens=np.full(B, cfg.T, np.int32),
                         labels=rng.integers(1, cfg.K + 1, B).astype(np.int32)))
    es = feat16.dtype_of(ft).itemsize
    ftk = {} if ft == "f32" else {"feat_type": ft}

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

    def questions(v, d):
        for k in ("tokens", "lens", "labels"):
            v[k][...] = d[k]

    def dense_into(v, d):                                # the host transpose and pad of one batch
        f = v["feats"]
        for i, (o, c) in enumerate(zip(d["off"], d["counts"])):
            f[i, :, :c] = d["rows"][o:o + c].T
            f[i, :, c:] = 0

    def rows_into(v, d):                                 # the concatenation a packed loader does
        v["feats"].reshape(-1)[:d["rows"].size] = d["rows"].reshape(-1)

    def dense_upload(sl, d):
        m.set_batch_async(sl, regions=d["counts"], **ftk)

    def packed_upload(sl, d):
        m.set_batch_async(sl, packed_counts=d["counts"], **ftk)

    def fresh(fill, upload):
        """ms/step: batch i+1 goes into the other slot under step i; fill = None: the staging is already filled."""
        def body(i):
            m.use_batch(i & 1)
            sl = (i + 1) & 1
            if fill is not None:
                fill(m.batch_slot(sl, **ftk), data[sl])
            upload(sl, data[sl])
            step(i)
        for sl in (0, 1):
            v = m.batch_slot(sl, **ftk)
            (dense_into if upload is dense_upload else rows_into)(v, data[sl])
            questions(v, data[sl])
        upload(0, data[0])
        m.use_batch(0)
        return round(timed(body, args.steps), 3)

    def alone(upload):
        def body(i):
            upload(i & 1, data[i & 1])
            m.use_batch(i & 1)
            m.sync()
        return round(timed(body, args.steps), 3)

    mean = float(np.mean([d["counts"].sum() for d in data]))
    out = {"B": B, "D": D, "S": S, "dtype": "bf16", "feat_type": ft, "steps": args.steps,
           "dense_bytes_per_step": B * D * S * es, "packed_bytes_per_step": int(mean * D * es),
           "link_fraction": round(mean / (B * S), 4)}
    if "a" in legs:
        out["dense_ms"] = fresh(None, dense_upload)
        out["dense_upload_ms"] = alone(dense_upload)
    if "b" in legs:
        out["dense_host_ms"] = fresh(dense_into, dense_upload)
    if "c" in legs:
        out["packed_ms"] = fresh(None, packed_upload)
        out["packed_upload_ms"] = alone(packed_upload)
    if "d" in legs:
        out["packed_host_ms"] = fresh(rows_into, packed_upload)
    if "c" in legs or "d" in legs:                       # the unpack launch alone
        m.sync()
        m.prof_enable(True)
        m.prof_reset()
        for i in range(args.prof_steps):
            packed_upload(i & 1, data[i & 1])
            m.use_batch(i & 1)
            m.sync()
        p = m.prof()["unpack_regions"]
        m.prof_enable(False)
        out["unpack_ms"] = round(p["ms"] / p["launches"], 4)
        out["unpack_GBps"] = round(p["bytes"] / p["ms"] / 1e6, 1)
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
