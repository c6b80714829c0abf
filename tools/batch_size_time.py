"""What rau_set_batch_size costs and what it buys, on one GPU.  Three measurements, one JSON line:

  resize    wall time of one rau_set_batch_size (it synchronises) down and back up, after a step has run, at
            configs[1] widths (D = 512, f32) for 100 -> 83 and 256 -> 96 and at D = 2048 in RAU_BF16 mode for
            80 -> 32; next to it the device memory the context holds (hipMemGetInfo before / after rau_create):
            the call clears all of it except parameters, gradients and optimizer state.
  step      evaluate-mode forward, and forward + rau_predict, at n = 83 and 96 on a context of 100 resized to n
            against a FRESH context of n created in this process: same kernels, same launch policy, so they
            should differ by no more than the fresh context's own spread.  Legs alternate --rounds times.
  replaces  one epoch boundary (train at 100, evaluate at 83, train again) at configs[1] widths with a bank of
            --bank-rows f16 maps: today's route -- a second context of 83 rows, the parameters copied through
            the host into it, a second bank filled with the same rows -- against two resizes of the one context;
            time and device memory of each.

    python tools/batch_size_time.py [--steps 30] [--warmup 3] [--rounds 5] [--bank-rows 2000]
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bank-rows", type=int, default=2000)
    ap.add_argument("--only", choices=["resize", "step", "replaces"], default=None)
    args = ap.parse_args()
    import torch  # before librau.so: one HIP runtime
    from rau_vqa_amd import synth
    from rau_vqa_amd.model import RAU, Config

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()     # hipMemGetInfo
        return total - free

    def stat(v, nd=3):
        return {"min": round(min(v), nd), "max": round(max(v), nd), "median": round(float(np.median(v)), nd)}

    def batch(cfg, n, seed=1):
        return synth.make_batch(n, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=seed)

    res = {"tool": "batch_size_time", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}

    # ---- the cost of one resize
    if args.only in (None, "resize"):
        res["resize_ms"] = {}
        for name, kw, cap, n in (("D512_f32_100_to_83", dict(D=512, dtype="f32"), 100, 83),
                                 ("D512_f32_256_to_96", dict(D=512, dtype="f32"), 256, 96),
                                 ("D2048_bf16_80_to_32", dict(D=2048, dtype="bf16"), 80, 32)):
            m0 = used()
            cfg = Config(B=cap, **kw)
            m = RAU(cfg)
            m.init_uniform(1, -0.08, 0.08)
            held = used() - m0
            hop_w = np.full(cfg.H, float(cfg.H), np.float32)
            bs = {cap: batch(cfg, cap), n: batch(cfg, n)}
            down, up = [], []
            for rnd in range(args.rounds + 1):
                for size, out in ((cap, down), (n, up)):     # a step at `size`, then the switch away from it
                    b = bs[size]
                    m.training()
                    m.set_dropout_seed(5, rnd)
                    m.set_batch(b["feats"], b["tokens"], b["lens"], b["labels"])
                    m.zero_grads()
                    m.forward()
                    m.backward(hop_w)
                    m.sync()
                    t0 = time.perf_counter()
                    m.set_batch_size(n if size == cap else cap)
                    if rnd:                                    # (round 0 warms up)
                        out.append((time.perf_counter() - t0) * 1e3)
            m.close()
            res["resize_ms"][name] = {"down": stat(down), "up": stat(up), "context_MB": round(held / 2**20, 1)}

    # ---- step time at the new size: resized against fresh
    if args.only in (None, "step"):
        res["eval_step_ms"] = {}
        for n in (83, 96):
            cfg = Config(B=100)
            legs = {"resized": RAU(cfg), "fresh": RAU(Config(B=n))}
            b = batch(cfg, n)
            mc = np.random.default_rng(3).integers(0, cfg.K + 1, (n, 18)).astype(np.int32)
            for m in legs.values():
                m.init_uniform(1, -0.08, 0.08)
                m.evaluate()
                m.set_batch(b["feats"], b["tokens"], b["lens"], None)      # (resizes the first)
            assert legs["resized"].batch_size == n == legs["fresh"].batch_size
            t = {k: {"forward": [], "forward_predict": []} for k in legs}

            def run(m, steps, predict):
                for _ in range(steps):
                    m.forward()
                    if predict:
                        m.predict(mc)
            for rnd in range(args.rounds):
                for k, m in legs.items():
                    for what, predict in (("forward", False), ("forward_predict", True)):
                        run(m, args.warmup, predict)
                        m.sync()
                        t0 = time.perf_counter()
                        run(m, args.steps, predict)
                        m.sync()
                        t[k][what].append((time.perf_counter() - t0) * 1e3 / args.steps)
            same = np.array_equal(legs["resized"].logits(), legs["fresh"].logits())
            for m in legs.values():
                m.close()
            res["eval_step_ms"][f"n{n}"] = {k: {w: dict(stat(v), all=[round(x, 3) for x in v]) for w, v in d.items()}
                                            for k, d in t.items()}
            res["eval_step_ms"][f"n{n}"]["logits_equal"] = bool(same)

    # ---- what it replaces: one epoch boundary
    if args.only in (None, "replaces"):
        cfg = Config(B=100)
        R = args.bank_rows
        maps = np.random.default_rng(4).standard_normal((R, cfg.D, cfg.S)).astype(np.float16)
        train = RAU(cfg)
        train.init_uniform(1, -0.08, 0.08)
        train.bank_create(R, "f16")
        train.bank_put(0, maps)
        train.sync()
        base = used()
        second_ms, second_mb, resize_ms, resize_mb = [], [], [], []
        for rnd in range(args.rounds):
            t0 = time.perf_counter()
            ev = RAU(Config(B=83))
            ev.set_params(train.get_params())
            ev.bank_create(R, "f16")
            ev.bank_put(0, maps)
            ev.evaluate()
            ev.sync()
            second_ms.append((time.perf_counter() - t0) * 1e3)
            second_mb.append((used() - base) / 2**20)
            ev.close()
            t0 = time.perf_counter()
            train.set_batch_size(83)
            train.evaluate()
            train.set_batch_size(100)
            train.training()
            resize_ms.append((time.perf_counter() - t0) * 1e3)
            train.set_batch_size(83)                 # (untimed: the memory while the context evaluates)
            resize_mb.append((used() - base) / 2**20)
            train.set_batch_size(100)
        train.close()
        res["epoch_boundary"] = {"bank_rows": R, "bank_MB": round(maps.nbytes / 2**20, 1),
                                 "second_context": {"ms": stat(second_ms, 1), "extra_device_MB": stat(second_mb, 1)},
                                 "two_resizes": {"ms": stat(resize_ms, 2), "extra_device_MB": stat(resize_mb, 1)}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
