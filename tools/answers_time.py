"""Cost of the VQA-metric scores of a step's answers: device vs host, one GPU.

configs[1] network (Ours_SS, 14x14x512, 8 hops, K = 1000) at B = 256 and 1024, evaluate mode, every sample with
an answer set of G = 10 entries (ids, weights count / 10, scores min(count / 3, 1)).  Per batch size:
  * scores_dev_ms   rau_step_scores (three launches + the download of [H+2, B] scores and H+2 totals), median of
                    --reps;
  * scores_host_ms  download logits [H,B,K] + dopred, then predict.set_stats in numpy (merges, first-max answers,
                    answer_score);
  * stats_dev_ms    rau_step_stats with the set (soft CE of the merged rows, the correct rule);
  * set_answers_ms  rau_set_answers on the resident batch (host checks + three copies + a synchronise).
One JSON line per batch size:

    python tools/answers_time.py [--batches 256 1024] [--reps 20]
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


def median_ms(fn, reps):
    fn()   # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--G", type=int, default=10)
    args = ap.parse_args()
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import loader, predict, synth
    from rau_vqa_amd.model import RAU, Config
    for B in args.batches:
        cfg = Config(B=B)
        m = RAU(cfg)
        m.init_uniform(1, -0.08, 0.08)
        batch = synth.make_batch(B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=1)
        rng = np.random.default_rng(1)
        ids = rng.integers(0, cfg.K + 1, size=(B, args.G)).astype(np.int32)
        counts = rng.integers(1, 11, size=(B, args.G))
        w, score = (counts / 10).astype(np.float32), loader.vqa_scores(counts)
        m.evaluate()
        m.set_batch(**batch)
        res = {"tool": "answers_time", "B": B, "H": cfg.H, "K": cfg.K, "G": args.G, "reps": args.reps}
        res["set_answers_ms"] = median_ms(lambda: m.set_answers(ids, w, score), args.reps)
        m.forward()
        m.sync()
        res["scores_dev_ms"] = median_ms(m.step_scores, args.reps)
        res["stats_dev_ms"] = median_ms(m.step_stats, args.reps)
        res["scores_host_ms"] = median_ms(
            lambda: predict.set_stats(m.logits(), m.dopred(), ids, w, score)["score"], args.reps)
        m.close()
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}),
              flush=True)


if __name__ == "__main__":
    main()
