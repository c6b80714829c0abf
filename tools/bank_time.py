"""Throughput of batches drawn from the device-resident feature bank against uploaded batches, on one GPU.

The workloads are those of tools/shared_images_time.py (--config 1: configs[1] widths, D = 512, f32;
--config 2: D = 2048 in RAU_BF16 mode) at batch size --batch.  For two kinds of batch -- `plain` (every
question its own image, N = B) and `third` (three questions per image, N = B/3) -- and the element types
f32 and f16 it times the evaluate-mode forward three ways:
  upload    today's path: a new batch goes up EVERY step through the two pinned upload slots (staging
            filled in place beforehand: the step pays the H2D copy and nothing else of a loader);
  bank      the maps are in the bank; every step names a DIFFERENT set of rows through the two slots
            (rau_set_batch_async_bank: the gather runs on the copy stream under the step in flight);
  resident  the batch already in HBM, nothing moved: the ceiling.
A training leg (forward + backward, f32 maps, plain batches) compares upload against bank the same way.
All legs run in this one process, alternated --rounds times, so a leg's spread against itself stands next
to the differences between legs.  Also reported: the bank gather's own time and bytes (rau_prof class
`bank_gather`, alone on the stream), rau_bank_put's rate with and without narrowing, and the fill time and
bytes of an e4m3 bank (f32 maps narrowed on the device) beside the f16 bank.  One JSON line:

    python tools/bank_time.py --config 1 --batch 256 [--steps 30] [--rounds 5]
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

WORKLOADS = {1: dict(name="configs[1] widths", D=512, dtype="f32"),
             2: dict(name="D=2048 bf16 mode", D=2048, dtype="bf16")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(WORKLOADS), required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=10)
    args = ap.parse_args()
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import synth
    from rau_vqa_amd.model import RAU, Config
    w = WORKLOADS[args.config]
    B = args.batch
    cfg = Config(B=B, D=w["D"], dtype=w["dtype"])
    m = RAU(cfg)
    m.init_uniform(1, -0.08, 0.08)
    b = synth.make_batch(B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=1)
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    N3 = (B + 2) // 3
    rng = np.random.default_rng(2)
    third = rng.permutation(np.arange(B) % N3).astype(np.int32)       # three questions per image, shuffled
    POOL = 2 * B                                                      # bank rows the steps draw from
    maps = {"f32": b["feats"], "f16": b["feats"].astype(np.float16)}
    kinds = {"plain": dict(n=B, image_of=None), "third": dict(n=N3, image_of=third)}
    nsteps = max(args.steps, args.train_steps) + args.warmup + 2
    rows = {k: [rng.permutation(POOL)[:v["n"]].astype(np.int32) for _ in range(nsteps)] for k, v in kinds.items()}

    put_gbs = {"f32_to_f32": [], "f16_to_f16": [], "f32_to_f16_narrowed": [], "f32_to_e4m3_narrowed": []}
    fill_ms = {"f16": [], "e4m3": []}          # wall time of filling POOL rows from f32 maps, per bank type

    def fill(ft, narrowed=False):
        """a fresh bank of POOL maps of `ft`, filled with two puts of B maps; records the rate"""
        m.bank_destroy()
        m.bank_create(POOL, ft)
        src = maps["f32"] if narrowed else maps[ft]
        t0 = time.perf_counter()
        m.bank_put(0, src)
        m.bank_put(B, src)
        dt = time.perf_counter() - t0
        put_gbs[f"f32_to_{ft}_narrowed" if narrowed else f"{ft}_to_{ft}"].append(2 * src.nbytes / dt / 1e9)
        if narrowed:
            fill_ms[ft].append(dt * 1e3)

    def stage(kind, ft):
        """the leg's batch into the pinned staging of both slots, in place"""
        n = kinds[kind]["n"]
        for s in (0, 1):
            v = m.batch_slot(s, ft)
            v["feats"].reshape(-1)[:n * cfg.D * cfg.S] = maps[ft][:n].reshape(-1)
            v["tokens"][...] = b["tokens"]
            v["lens"][...] = b["lens"]
            v["labels"][...] = b["labels"]

    cur = [0]                                 # the resident slot (a forward's batch cannot be refilled in place)

    def step(train):
        if train:
            m.zero_grads()
            m.forward()
            m.backward(hop_w)
        else:
            m.forward()

    def upload(kind, ft, steps, train=False):
        k = kinds[kind]
        table = {} if k["image_of"] is None else {"image_of": k["image_of"], "n_images": k["n"]}
        for i in range(steps + 1):            # upload i + 1 is enqueued while step i runs
            s = cur[0] ^ 1
            m.set_batch_async(s, has_labels=train, feat_type=ft, **table)
            m.use_batch(s)
            cur[0] = s
            if i < steps:
                step(train)

    def bank(kind, ft, steps, train=False):
        k = kinds[kind]
        for i in range(steps + 1):
            s = cur[0] ^ 1
            m.set_batch_async(s, has_labels=train, bank_rows=rows[kind][i], image_of=k["image_of"])
            m.use_batch(s)
            cur[0] = s
            if i < steps:
                step(train)

    def resident(kind, ft, steps, train=False):
        for _ in range(steps):
            step(train)

    def timed(fn, kind, ft, steps, train=False):
        fn(kind, ft, args.warmup, train)
        m.sync()
        t0 = time.perf_counter()
        fn(kind, ft, steps, train)
        m.sync()
        return B * steps / (time.perf_counter() - t0)

    legs = [(k, ft) for k in kinds for ft in ("f32", "f16")]
    qa = {f"{k}_{ft}": {"upload": [], "bank": [], "resident": []} for k, ft in legs}
    tr = {"upload": [], "bank": []}
    gather = {}
    for rnd in range(args.rounds):
        m.evaluate()
        for ft in ("f32", "f16"):
            fill(ft)
            for k in kinds:
                stage(k, ft)
                qa[f"{k}_{ft}"]["upload"].append(timed(upload, k, ft, args.steps))
                qa[f"{k}_{ft}"]["bank"].append(timed(bank, k, ft, args.steps))
                kw = {} if kinds[k]["image_of"] is None else {"image_of": kinds[k]["image_of"]}
                m.set_batch(maps[ft][:kinds[k]["n"]], b["tokens"], b["lens"], None, **kw)
                qa[f"{k}_{ft}"]["resident"].append(timed(resident, k, ft, args.steps))
                if rnd == 0:                  # the gather alone on the chain stream, bracketed by events
                    m.prof_enable(True)
                    m.prof_reset()
                    for i in range(10):
                        m.set_batch(None, b["tokens"], b["lens"], None, bank_rows=rows[k][i],
                                    image_of=kinds[k]["image_of"])
                    p = m.prof()["bank_gather"]
                    m.prof_enable(False)
                    gather[f"{k}_{ft}"] = {"ms": round(p["ms"] / p["launches"], 4),
                                           "bytes_moved": p["bytes"] / p["launches"],
                                           "GB_s": round(p["bytes"] / p["launches"] / (p["ms"] / p["launches"]) / 1e6, 1)}
        fill("f16", narrowed=True)
        fill("e4m3", narrowed=True)
        # training: forward + backward on plain f32 batches, Philox masks
        m.training()
        m.set_dropout_seed(5, rnd)
        fill("f32")
        stage("plain", "f32")
        tr["upload"].append(timed(upload, "plain", "f32", args.train_steps, True))
        tr["bank"].append(timed(bank, "plain", "f32", args.train_steps, True))
    m.close()

    def summary(v):
        return {"kqa_s": [round(x / 1e3, 2) for x in v], "min": round(min(v) / 1e3, 2), "max": round(max(v) / 1e3, 2),
                "median": round(float(np.median(v)) / 1e3, 2)}
    res = {"tool": "bank_time", "workload": w["name"], "B": B, "D": cfg.D, "S": cfg.S, "H": cfg.H, "steps": args.steps,
           "train_steps": args.train_steps, "rounds": args.rounds, "pool_rows": POOL,
           "eval": {k: {leg: summary(v) for leg, v in d.items()} for k, d in qa.items()},
           "train_plain_f32": {leg: summary(v) for leg, v in tr.items()},
           "bank_gather": gather,
           "bank_fill_from_f32": {ft: {"rows": POOL, "bank_bytes": POOL * cfg.D * cfg.S * (2 if ft == "f16" else 1),
                                       "ms_min": round(min(v), 2), "ms_median": round(float(np.median(v)), 2)}
                                  for ft, v in fill_ms.items()},
           "bank_put_GB_s": {k: {"min": round(min(v), 2), "max": round(max(v), 2), "median": round(float(np.median(v)), 2)}
                             for k, v in put_gbs.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
