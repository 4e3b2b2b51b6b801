"""Microbenchmark of the batched sampler (roma_amd.sample_matches / RegressionMatcher.sample_batched, csrc/sample_batched.hip)
against what it replaces, the Python loop of one RegressionMatcher.sample call per pair, at the size match() produces:
B = 8 pairs of n = 864 x 1728 rows (a symmetric 864 warp) on a synthetic certainty map, num = 10 000 and 5 000.

Both legs run in one process on the same tensors, timed alternately with device events: --rounds rounds (7) of --iters calls (20)
per leg, medians and spread over the rounds.  One JSON line per num, appended to --out (profiles/sample_batched_bench.jsonl) and
printed.  The loop's code is the single-pair path this library has always had, so its leg stands for the library without the
batched sampler.  --only batched runs that leg alone (for a kernel trace in a run of its own).
Usage: python tools/bench_sample.py [--iters 20] [--rounds 7] [--num 10000 5000] [--only batched|loop] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def synthetic_warp(B, H=864, W=1728, seed=0):
    """(warp [B, H, W, 4], certainty [B, H, W]) on the device: a smooth flow over the pixel grid and a certainty map of smooth
    blobs, zero over most of the frame and above sample_thresh over about a fifth of it, as a real pair's is"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = ((torch.arange(H, device=DEV) + 0.5) / H * 2 - 1)[None, :, None].expand(B, H, W)
    x = ((torch.arange(W, device=DEV) + 0.5) / W * 2 - 1)[None, None, :].expand(B, H, W)
    ph = torch.arange(B, device=DEV, dtype=torch.float32)[:, None, None]
    warp = torch.stack((x, y, x + 0.1 * torch.sin(3 * y + ph), y + 0.1 * torch.cos(2 * x + ph)), -1).contiguous()
    blobs = torch.sin(5 * x + ph) * torch.cos(4 * y + 0.3 * ph)
    cert = (blobs.clamp(min=0) ** 2 * (torch.rand((B, H, W), device=DEV, generator=g) > 0.4) * (blobs > 0.25)).contiguous()
    return warp, cert


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--num", type=int, nargs="+", default=[10000, 5000])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--only", choices=("batched", "loop"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_batched_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample.py measures the device path: it needs a GPU"
    from roma_amd.matcher import RegressionMatcher
    m = RegressionMatcher.__new__(RegressionMatcher)  # the two sampling methods need only these attributes
    m.sample_mode, m.sample_thresh = "threshold_balanced", 0.05
    B = args.batch
    warp, cert = synthetic_warp(B)
    seeds = torch.arange(B, dtype=torch.int64) + 1
    for num in args.num:
        legs = {"batched ms": lambda: m.sample_batched(warp, cert, num=num, seed=seeds, return_counts=True),
                "loop ms": lambda: [m.sample(warp[b], cert[b], num=num) for b in range(B)]}
        if args.only:
            legs = {k: v for k, v in legs.items() if k.startswith(args.only)}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k].append(timed(fn, args.iters))
        res = {"config": "sample threshold_balanced", "B": B, "n": int(cert[0].numel()), "num": num,
               "certain_fraction": round(float((cert > 0.05).float().mean()), 4), "rounds": args.rounds, "iters_per_round": args.iters,
               **{k: stats(v) for k, v in ms.items()}}
        if len(legs) == 2:
            loop, bat = ms["loop ms"], ms["batched ms"]
            res["loop over batched"] = round(float(np.median(loop) / np.median(bat)), 3)
            res["batched within the loop's median minus its spread"] = bool(np.median(bat) <= np.median(loop) - (np.max(loop) - np.min(loop)))
            counts = legs["batched ms"]()[2]
            res["counts"] = counts.cpu().tolist()
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
