"""Evaluate-mode throughput with batches that share feature maps between questions, on one GPU.

For one workload (--config 1: configs[1] widths, D = 512, f32; --config 2: D = 2048 in RAU_BF16 mode) at
batch size --batch it times the evaluate-mode forward (rau_forward, all hops) over four kinds of batch:
  a  plain            feats [B,D,S] f32, one map per question (today's path);
  b  table N = B      the same maps as an image table with a permutation index: the cost of the indexed read;
  c  table N = B/3    three questions per image (VQA v1), f32 maps;
  d  table N = B/3    the same with f16 maps.
Each leg is measured two ways: `fresh` = a new batch uploaded EVERY step through the two pinned upload
slots (staging filled in place beforehand, so the step pays the H2D copy and nothing else of the loader),
and `resident` = the batch already in HBM.  All legs run in this one process, alternated --rounds times,
so the spread of a leg against itself is visible next to the differences between legs.  The line also
carries the byte and FLOP ratios the shapes give: feature bytes over the link, and the two hoisted
convolutions' FLOP, each relative to leg a.  One JSON line per run:

    python tools/shared_images_time.py --config 1 --batch 256 [--steps 30] [--rounds 5]
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
    args = ap.parse_args()
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import synth
    from rau_vqa_amd.model import RAU, Config
    w = WORKLOADS[args.config]
    B = args.batch
    cfg = Config(B=B, D=w["D"], dtype=w["dtype"])
    m = RAU(cfg)
    m.init_uniform(1, -0.08, 0.08)
    m.evaluate()
    b = synth.make_batch(B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=1)
    N3 = (B + 2) // 3
    rng = np.random.default_rng(2)
    third = rng.permutation(np.arange(B) % N3).astype(np.int32)       # three questions per image, shuffled
    legs = {
        "a_plain": dict(feats=b["feats"], ft="f32", image_of=None),
        "b_table_N=B": dict(feats=b["feats"], ft="f32", image_of=rng.permutation(B).astype(np.int32)),
        "c_table_N=B/3": dict(feats=b["feats"][:N3], ft="f32", image_of=third),
        "d_table_N=B/3_f16": dict(feats=b["feats"][:N3].astype(np.float16), ft="f16", image_of=third),
    }

    def table_args(leg):
        return {} if leg["image_of"] is None else {"image_of": leg["image_of"], "n_images": len(leg["feats"])}

    def stage(leg):
        """the leg's batch into the pinned staging of both slots, in place"""
        for s in (0, 1):
            v = m.batch_slot(s, leg["ft"])
            v["feats"].reshape(-1)[:leg["feats"].size] = leg["feats"].reshape(-1)
            v["tokens"][...] = b["tokens"]
            v["lens"][...] = b["lens"]

    cur = [0]                                 # the resident slot (a forward's batch cannot be refilled in place)

    def fresh(leg, steps):
        for i in range(steps + 1):            # upload i + 1 is enqueued while forward i runs
            s = cur[0] ^ 1
            m.set_batch_async(s, has_labels=False, feat_type=leg["ft"], **table_args(leg))
            m.use_batch(s)
            cur[0] = s
            if i < steps:
                m.forward()

    def resident(leg, steps):
        for _ in range(steps):
            m.forward()

    def timed(fn, leg):
        fn(leg, args.warmup)
        m.sync()
        t0 = time.perf_counter()
        fn(leg, args.steps)
        m.sync()
        return B * args.steps / (time.perf_counter() - t0)

    qa = {k: {"fresh": [], "resident": []} for k in legs}
    for _ in range(args.rounds):
        for k, leg in legs.items():
            stage(leg)
            qa[k]["fresh"].append(timed(fresh, leg))
        for k, leg in legs.items():
            m.set_batch(leg["feats"], b["tokens"], b["lens"], None, feat_type=leg["ft"], image_of=leg["image_of"])
            qa[k]["resident"].append(timed(resident, leg))
    m.close()
    es = {"f32": 4, "f16": 2}
    base_bytes = legs["a_plain"]["feats"].size * 4
    res = {"tool": "shared_images_time", "workload": w["name"], "B": B, "D": cfg.D, "S": cfg.S, "H": cfg.H,
           "steps": args.steps, "rounds": args.rounds, "legs": {}}
    for k, leg in legs.items():
        n = len(leg["feats"])
        res["legs"][k] = {
            "n_maps": n,
            "feat_bytes_ratio": round(leg["feats"].size * es[leg["ft"]] / base_bytes, 4),
            "conv_flop_ratio": round(n / B, 4),
            "fresh_kqa_s": [round(v / 1e3, 2) for v in qa[k]["fresh"]],
            "resident_kqa_s": [round(v / 1e3, 2) for v in qa[k]["resident"]],
            "fresh_median_kqa_s": round(float(np.median(qa[k]["fresh"])) / 1e3, 2),
            "resident_median_kqa_s": round(float(np.median(qa[k]["resident"])) / 1e3, 2),
        }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
