"""Cost of ranked answers with confidences: rau_topk on the device vs the download route, one GPU.

configs[1] network (Ours_SS, 14x14x512, 8 hops, K = 1000) at B = 256 and 1024, evaluate mode, after
one forward (the part after the forward alone, as tools/hop_merge_time.py's merge_* columns).  Per
batch size and per k in --ks:
  * topk_dev_ms   RAU.topk(k): one launch, [H+2, B, k] ids + scores + confidences downloaded;
  * topk_host_ms  the only route without it: rau_get_logits ([H, B, K] floats) + do_pred,
                  predict.merge_hops (on a one-column dummy for the attention maps, which are not
                  downloaded), then a numpy top-k: argpartition + a sort of the k, softmax of the row
                  for the confidences -- the fast way, not predict.top_answers' full stable sort, so
                  that the comparison does not flatter the device.
Medians of --reps, one JSON line per batch size:

    python tools/topk_time.py [--batches 256 1024] [--ks 1 5 10] [--reps 20]
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


def numpy_topk(tab_pred, k):
    """ids (1-based), scores, confidences [R, B, k] the quick way (ties in no particular order)"""
    x = np.stack(tab_pred)
    K = x.shape[-1]
    part = np.argpartition(x, K - k, axis=-1)[..., K - k:]
    order = np.argsort(-np.take_along_axis(x, part, -1), axis=-1)
    ids = np.take_along_axis(part, order, -1)
    score = np.take_along_axis(x, ids, -1)
    mx = score[..., :1]
    conf = np.exp(score - mx) / np.exp(x - mx).sum(-1, keepdims=True)
    return ids.astype(np.int32) + 1, score, conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 5, 10])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch  # noqa: F401  (before librau.so: one HIP runtime)
    from rau_vqa_amd import predict, synth
    from rau_vqa_amd.model import RAU, Config
    for B in args.batches:
        cfg = Config(B=B)
        m = RAU(cfg)
        m.init_uniform(1, -0.08, 0.08)
        batch = synth.make_batch(B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=1)
        m.evaluate()
        m.set_batch(**batch)
        m.forward()
        m.sync()
        att0 = np.zeros((cfg.H, B, 1), np.float32)
        host = lambda k: numpy_topk(predict.merge_hops(m.logits(), m.dopred(), att0)[0], k)
        res = {"tool": "topk_time", "B": B, "H": cfg.H, "K": cfg.K, "reps": args.reps}
        for k in args.ks:
            res[f"topk_dev_ms_k{k}"] = median_ms(lambda: m.topk(k), args.reps)
            res[f"topk_host_ms_k{k}"] = median_ms(lambda: host(k), args.reps)
        # the two routes rank the same values (ids may differ where a row has a tie)
        res["scores_agree"] = bool(np.array_equal(m.topk(max(args.ks))[1], host(max(args.ks))[1]))
        m.close()
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}),
              flush=True)


if __name__ == "__main__":
    main()
