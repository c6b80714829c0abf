"""Cost of feval's joint-loss statistics and of predict_result's merges: device vs host, one GPU.

configs[1] network (Ours_SS, 14x14x512, 8 hops, K = 1000) at B = 256 and 1024, evaluate mode (the
hop outputs are what a training step leaves; dropout changes nothing here).  Per batch size:
  * stats_dev_ms      rau_step_stats (two launches + one 500-byte download), median of --reps;
  * stats_host_ms     download logits [H,B,K] + dopred, then joint.feval_stats in numpy;
  * predict_dev_ms    predict.predict_result_device (forward + rau_predict + merged rows + per-hop
                      logits / maps for tab_pred / tab_att, as predict_result returns them);
  * predict_dev_answers_ms  the same with tabs=False (answers only, no [H,B,K] download);
  * predict_host_ms   predict.predict_result (forward + downloads + numpy merges + MC loop);
  * merge_dev_ms / merge_host_ms  the part after the forward alone: rau_predict vs the downloads
                      + merge_hops + answers.
MC lists are [B, 18] (the reference's nMultChoice).  One JSON line per batch size:

    python tools/hop_merge_time.py [--batches 256 1024] [--reps 20]
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
    args = ap.parse_args()
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import joint, predict, synth
    from rau_vqa_amd.model import RAU, Config
    for B in args.batches:
        cfg = Config(B=B)
        m = RAU(cfg)
        m.init_uniform(1, -0.08, 0.08)
        batch = synth.make_batch(B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=1)
        mc = np.random.default_rng(1).integers(1, cfg.K + 1, size=(B, 18)).astype(np.int32)
        m.evaluate()
        m.set_batch(**batch)
        m.forward()
        m.sync()
        res = {"tool": "hop_merge_time", "B": B, "H": cfg.H, "K": cfg.K, "reps": args.reps}
        res["stats_dev_ms"] = median_ms(m.step_stats, args.reps)
        res["stats_host_ms"] = median_ms(
            lambda: joint.feval_stats(m.logits(), m.dopred(), batch["labels"]), args.reps)
        res["merge_dev_ms"] = median_ms(lambda: m.predict(mc), args.reps)
        res["merge_host_ms"] = median_ms(
            lambda: predict.answers(predict.merge_hops(m.logits(), m.dopred(), m.attention())[0], mc),
            args.reps)
        f, t, n = batch["feats"], batch["tokens"], batch["lens"]
        res["predict_dev_ms"] = median_ms(lambda: predict.predict_result_device(m, f, t, n, mc), args.reps)
        res["predict_dev_answers_ms"] = median_ms(
            lambda: predict.predict_result_device(m, f, t, n, mc, tabs=False), args.reps)
        res["predict_host_ms"] = median_ms(lambda: predict.predict_result(m, f, t, n, mc), args.reps)
        m.close()
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}),
              flush=True)


if __name__ == "__main__":
    main()
