"""Cost of the per-image feature-map gradient (rau_set_feat_grad, RAU_FEAT_GRAD_IMAGES) against the route it
replaces, one GPU.

At bench.py's configs[1] (B = 256, D = 512, f32) and configs[2] (B = 256, D = 2048, bf16) widths, three questions per
image (N = 86 images, image_of[b] = b // 3), training mode, device-drawn masks.  The image table [N,D,S] lives in a
torch CUDA tensor, as the output of a trained stage in front of the library would; a step ends with the gradient at
the TABLE in device memory and a synchronisation at the end of the timed window.  Legs:
  * off_ms       zero_grads + forward + backward of a resident plain batch, the switch off;
  * samples_ms   the same with mode 1 (RAU_FEAT_GRAD_SAMPLES);
  * expand_ms    the route this feature replaces, which needs nothing new: mode 1, x = table[image_of] formed in
                 torch, set_batch_dev(x), the step, index_add_ of the [B,D,S] result back to [N,D,S];
  * images_ms    the new route: mode 2, set_batch_dev(table, image_of=), the step; the result IS [N,D,S].
The first three also run on ANOTHER build of the library given with --parent-lib (the commit before this feature,
built by the caller: it is not part of the tree), as a child process of its own before and after this build's: off and
samples launch what they launched there and must sit inside the parent's own run-to-run spread.
Method: every leg is warmed up, then timed over --steps steps, --rounds times, the legs alternating inside one process;
reported per leg: the median of the rounds and their spread (max - min).  One JSON line per config:

    python tools/featgrad_images_time.py [--parent-lib PATH] [--configs 1 2] [--steps 20] [--rounds 5] [--warmup 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {1: dict(D=512, dtype="f32"), 2: dict(D=2048, dtype="bf16")}   # bench.py: configs[1], configs[2]
TAG = "FEATGRAD_IMAGES_TIME "
B, PER_IMAGE = 256, 3
N = (B + PER_IMAGE - 1) // PER_IMAGE


def child(args):
    import torch
    from rau_vqa_amd import _lib as L
    from rau_vqa_amd import synth
    from rau_vqa_amd.dist import device_view
    from rau_vqa_amd.model import RAU, Config
    c = CONFIGS[args.config]
    cfg = Config(B=B, T=26, V=14000, E=200, Rq=512, D=c["D"], S=196, M=512, A=256, R=512, K=1000, H=8,
                 dtype=c["dtype"])
    m = RAU(cfg)
    m.init_uniform(seed=123)
    batch = synth.make_batch(cfg.B, cfg.T, cfg.V, cfg.D, cfg.S, cfg.K, seed=123, lens="full")
    tok = (batch["tokens"], batch["lens"], batch["labels"])
    image_of = (np.arange(B) // PER_IMAGE).astype(np.int32)
    table = torch.as_tensor(np.ascontiguousarray(batch["feats"][:N])).cuda()
    idx = torch.as_tensor(image_of).long().cuda()
    m.set_batch(**batch)
    m.training()
    hop_w = np.full(cfg.H, float(cfg.H), np.float32)
    own = torch.cuda.ExternalStream(m.stream())
    cur = torch.cuda.current_stream()
    n = [0]
    state = {"leg": None}
    keep = {}

    def enter(leg):
        if state["leg"] == leg:
            return
        state["leg"] = leg
        mode = {"off": 0, "samples": 1, "expand": 1, "images": 2}[leg]
        L.check(m._lib.rau_set_feat_grad(m._h, mode))
        if leg in ("off", "samples"):
            m.set_batch(**batch)

    def core():
        m.set_dropout_seed(123, n[0])
        n[0] += 1
        m.zero_grads()
        m.forward()
        m.backward(hop_w)

    def step(leg):
        if leg == "expand":
            x = table[idx]                                      # [B,D,S] formed in torch
            own.wait_stream(cur)
            m.set_batch_dev(x, *tok)
            core()
            cur.wait_stream(own)
            p, pitch = C.c_void_p(), C.c_int32()
            L.check(m._lib.rau_feat_grad_dev(m._h, C.byref(p), C.byref(pitch)))
            g = device_view(p.value, B * cfg.D * pitch.value, cfg.device_id).view(B, cfg.D, pitch.value)[:, :, :cfg.S]
            keep["dT"] = torch.zeros_like(table).index_add_(0, idx, g)
            own.wait_stream(cur)
        elif leg == "images":
            own.wait_stream(cur)
            m.set_batch_dev(table, *tok, image_of=image_of)
            core()
            cur.wait_stream(own)
            keep["dT"] = m.feature_grad_tensor()                # [N,D,S], the library's buffer
        else:
            core()

    def timed(leg):
        enter(leg)
        for _ in range(args.warmup):
            step(leg)
        m.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(leg)
        m.sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    legs = ["off", "samples", "expand"] + (["images"] if args.leg == "this" else [])
    out = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            out[leg].append(round(timed(leg), 4))
    if args.leg == "this":    # the two routes end with the same gradient (the sum's order differs: not the same bits)
        enter("expand"); step("expand"); torch.cuda.synchronize(); a = keep["dT"].clone()
        n[0] -= 1
        enter("images"); step("images"); torch.cuda.synchronize(); b = keep["dT"]
        out["routes_rel_diff"] = float((a - b).abs().max() / a.abs().max())
    m.close()
    print(TAG + json.dumps(out), flush=True)


def run_child(args, config, leg, lib=None):
    env = dict(os.environ)
    if lib:
        env["RAU_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--config", str(config), "--steps",
           str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"child {leg} (config {config}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    for line in p.stdout.splitlines():
        if line.startswith(TAG):
            return json.loads(line[len(TAG):])
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
    ap.add_argument("--leg", default=None, help="(internal) run one child leg")
    ap.add_argument("--config", type=int, default=1, help="(internal)")
    args = ap.parse_args()
    if args.leg:
        return child(args)
    for config in args.configs:
        res = {"tool": "featgrad_images_time", "config": f"configs[{config}]", **CONFIGS[config], "B": B, "N": N,
               "H": 8, "steps": args.steps}
        before = run_child(args, config, "parent", args.parent_lib) if args.parent_lib else None
        r = run_child(args, config, "this")
        for leg in ("off", "samples", "expand", "images"):
            res[leg] = summary(r[leg])
        res["routes_rel_diff"] = r["routes_rel_diff"]
        if args.parent_lib:
            after = run_child(args, config, "parent", args.parent_lib)
            for leg in ("off", "samples", "expand"):
                par = summary(before[leg] + after[leg])
                res["parent_" + leg] = par
                d = res[leg]["median_ms"] - par["median_ms"]
                res[leg + "_minus_parent_ms"] = round(d, 4)
                res[leg + "_inside_parent_spread"] = bool(abs(d) <= par["spread_ms"])
        gain = res["expand"]["median_ms"] - res["images"]["median_ms"]
        res["images_gain_ms"] = round(gain, 4)
        res["images_beats_expand"] = bool(gain > max(res["expand"]["spread_ms"], res["images"]["spread_ms"]))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
