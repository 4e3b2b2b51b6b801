"""Benchmark of the on-device dense metrics (roma_amd.dense_metrics, csrc/gt_warp.hip) against the torch restatement of the
reference's geometric_dist that tools/accuracy_harness.py keeps as its second opinion, on the shape of the dense MegaDepth benchmark:
B = 8 pairs, a 560 x 560 warp scored over 384 x 512 depth maps.
  A  torch   accuracy_harness.geometric_dist on the device: grid_sample, inverse, batched matmuls, boolean indexing (about two dozen
             framework launches and a compaction that synchronises);
  B  hip     one roma_amd.dense_metrics call (two launches, nothing read back).
Both legs run interleaved (A B A B) in one process after a warm-up; each leg is a host clock around work that ends in a device
synchronise; median and min - max over --rounds rounds.  The work is launch-bound at this shape, so what is compared is the launch
count and the missing synchronisation, not bandwidth.  The two legs' results are compared (counts exactly, EPE to the summation
bound).  One JSON line, appended to --out (profiles/gt_warp_bench.jsonl) and printed.  Reported, not gated.
Usage: python tools/bench_gt_warp.py [--rounds 7] [--batch 8] [--res 560] [--depth 384 512]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEV = "cuda:0"


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=560)
    ap.add_argument("--depth", type=int, nargs=2, default=[384, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_warp_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gt_warp.py measures the device path: it needs a GPU"
    assert args.rounds >= 7, "at least 7 rounds"
    import roma_amd
    import accuracy_harness as AH
    dh, dw = args.depth
    data = {k: v.to(DEV) for k, v in AH.synthetic_planar_batch(args.batch, dh, dw, seed=0).items() if "depth" in k or k[0] in "TK"}
    pair = (data["im_A_depth"], data["im_B_depth"], data["T_1to2"], data["K1"], data["K2"])
    # a warp as a matcher returns it: the pixel centres of the res x res grid and the true coordinates plus about a pixel of noise
    x2, _ = roma_amd.get_gt_warp(*pair, H=args.res, W=args.res)
    ys, xs = torch.meshgrid(*(torch.linspace(-1 + 1 / args.res, 1 - 1 / args.res, args.res, device=DEV),) * 2, indexing="ij")
    grid = torch.stack((xs, ys), dim=-1)[None].expand(args.batch, -1, -1, -1)
    noise = torch.randn(x2.shape, generator=torch.Generator(DEV).manual_seed(0), device=DEV) * (2.0 / args.res)
    matches = torch.cat((grid, (x2 + noise).float()), dim=-1).contiguous()

    def leg_torch():
        return AH.geometric_dist(*pair, matches)

    def leg_hip():
        return roma_amd.dense_metrics(matches, *pair)

    for fn in (leg_torch, leg_hip, leg_torch, leg_hip):  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    ms = {"torch ms": [], "hip ms": []}
    for _ in range(args.rounds):
        for key, fn in (("torch ms", leg_torch), ("hip ms", leg_hip)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    gd, p1, p3, p5, prob = leg_torch()
    m = leg_hip()
    n = int(m.n_valid.sum())
    res = {"config": "gt_warp", "batch": args.batch, "warp": [args.res, args.res], "depth": [dh, dw], "rounds": args.rounds,
           **{k: stats(v) for k, v in ms.items()},
           "torch over hip": round(float(np.median(ms["torch ms"]) / np.median(ms["hip ms"])), 2),
           "hip faster than torch in every round": bool(np.max(ms["hip ms"]) < np.min(ms["torch ms"])),
           "valid pixels": [int(gd.numel()), n], "epe": [float(gd.mean()), float(m.epe)],
           "pck": [[float(p1), float(p3), float(p5)], [float(x) for x in m.pck]],
           "counts equal": bool(int(gd.numel()) == n and [int((gd < t).sum()) for t in (1.0, 3.0, 5.0)] == m.n_below.sum(dim=0).tolist())}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
