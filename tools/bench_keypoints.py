"""Benchmark of the batched on-device keypoint matching (roma_amd.match_keypoints, csrc/keypoints_batched.hip) on B pairs of N x N
detector keypoints over 560 x 560 warps - B = 8 with 4096 and 8192 keypoints per image, and B = 1 with 8192:
  A  loop    the single-pair RegressionMatcher.match_keypoints once per pair: per pair six kernels and two memsets (48 + 16 at B = 8),
             five allocations and one host read of the pair count between the count and the fill;
  B  batched one roma_amd.match_keypoints call: five launches whatever B is, nothing read back;
  C  torch   the reference's route kept on the device, per pair: F.grid_sample of warp and certainty, torch.cdist, the mask of
             matcher.py:756-762 and torch.nonzero (which synchronises).
The three legs run interleaved (A B C A B C) in one process after a warm-up; a round of a leg is a host clock around --inner calls
that end in one device synchronise, reported per call; median and min - max over --rounds rounds.  Legs A and B must return the same
pairs (checked, index for index); leg C's pair count is reported next to theirs.  One JSON line per shape, appended to --out
(profiles/keypoints_bench.jsonl) and printed.  Reported, not gated.
Usage: python tools/bench_keypoints.py [--rounds 9] [--inner 5] [--shapes b8_4096 b8_8192 b1_8192]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
SIDE = 560
SHAPES = {"b8_4096": dict(B=8, N=4096), "b8_8192": dict(B=8, N=8192), "b1_8192": dict(B=1, N=8192)}
LAUNCHES_PER_PAIR_LOOP = 8  # sample_warp_at, two memsets, nn x 2, count, scan, fill
LAUNCHES_BATCHED = 5


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def synthetic_scene(B, N, seed=0):
    """seeded smooth warps [B, 560, 560, 4] with a certainty that falls off towards the corners, N keypoints of A per pair, and
    N keypoints of B: 60 % the warped keypoints of A with 0.002 of noise, the rest uniform; shuffled"""
    ys = torch.linspace(-1 + 1 / SIDE, 1 - 1 / SIDE, SIDE, device=DEV, dtype=torch.float64)
    y, x = torch.meshgrid(ys, ys, indexing="ij")
    g = torch.Generator("cpu").manual_seed(seed)
    warps, certs, xa, xb = [], [], [], []
    for _ in range(B):
        p = torch.rand(6, generator=g, dtype=torch.float64).tolist()
        bx = 0.9 * x + 0.08 * torch.sin(3.0 * y + 6.0 * p[0]) + 0.06 * (p[1] - 0.5)
        by = 0.85 * y - 0.06 * torch.cos(2.0 * x + 6.0 * p[2]) + 0.06 * (p[3] - 0.5)
        warp = torch.stack((x, y, bx, by), dim=-1).float()
        cert = torch.sigmoid(4.0 * (1.0 - (x ** 2 + y ** 2))).float()
        a = (torch.rand((N, 2), generator=g) * 1.9 - 0.95).to(DEV)
        moved = F.grid_sample(warp[..., 2:].permute(2, 0, 1)[None], a[None, None], align_corners=False, mode="bilinear")[0, :, 0].mT
        n_near = N * 6 // 10
        b = torch.cat([moved[:n_near] + 0.002 * torch.randn((n_near, 2), generator=g).to(DEV), (torch.rand((N - n_near, 2), generator=g) * 2 - 1).to(DEV)])
        warps.append(warp), certs.append(cert), xa.append(a), xb.append(b[torch.randperm(N, generator=g).to(DEV)])
    return torch.stack(warps).contiguous(), torch.stack(certs).contiguous(), torch.stack(xa).contiguous(), torch.stack(xb).contiguous()


def torch_route(x_a, x_b, warp, cert, max_dist=0.005, cert_th=0):
    """matcher.py:732-773 for one pair, on the device"""
    p = F.grid_sample(warp[..., -2:].permute(2, 0, 1)[None], x_a[None, None], align_corners=False, mode="bilinear")[0, :, 0].mT
    c = F.grid_sample(cert[None, None], x_a[None, None], align_corners=False, mode="bilinear")[0, 0, 0]
    D = torch.cdist(p, x_b)
    return torch.nonzero((D == D.min(dim=-1, keepdim=True).values) * (D == D.min(dim=-2, keepdim=True).values) * (c[:, None] > cert_th)
                         * (D < max_dist), as_tuple=True)


def run(name, shape, rounds, inner):
    import roma_amd
    from roma_amd.matcher import RegressionMatcher
    B, N = shape["B"], shape["N"]
    warp, cert, xa, xb = synthetic_scene(B, N)
    m = RegressionMatcher.__new__(RegressionMatcher)

    def leg_loop():
        return [m.match_keypoints(xa[b], xb[b], warp[b], cert[b], return_inds=True) for b in range(B)]

    def leg_batched():
        return roma_amd.match_keypoints(xa, xb, warp, cert)

    def leg_torch():
        return [torch_route(xa[b], xb[b], warp[b], cert[b]) for b in range(B)]

    legs = (("loop ms", leg_loop), ("batched ms", leg_batched), ("torch ms", leg_torch))
    for _ in range(2):  # warm-up: code objects, allocator
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in legs}
    for _ in range(rounds):
        for key, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3 / inner)
    # legs A and B return the same pairs
    got, ref, tor = leg_batched(), leg_loop(), leg_torch()
    torch.cuda.synchronize()
    counts, total = got.counts.tolist(), got.total.tolist()
    same = counts == total
    for b in range(B):
        pairs = torch.stack(ref[b], dim=-1)
        same = same and len(pairs) == counts[b] and bool((got.inds[b, :counts[b]].long() == pairs).all()) and bool((got.inds[b, counts[b]:] == -1).all())
    loop_med, batched_med = float(np.median(ms["loop ms"])), float(np.median(ms["batched ms"]))
    return {"config": "keypoints", "shape": name, "batch": B, "keypoints per image": N, "warp": [SIDE, SIDE], "rounds": rounds,
            "calls per round": inner, **{k: stats(v) for k, v in ms.items()},
            "loop over batched": round(loop_med / batched_med, 2),
            "torch over batched": round(float(np.median(ms["torch ms"])) / batched_med, 2),
            "batched faster than loop in every round": bool(np.max(ms["batched ms"]) < np.min(ms["loop ms"])),
            "launches loop": LAUNCHES_PER_PAIR_LOOP * B, "host reads loop": B, "launches batched": LAUNCHES_BATCHED, "host reads batched": 0,
            "launches torch": "framework-internal, not counted", "host reads torch": B,
            "pairs per pair of images": total, "torch pairs": [int(len(t[0])) for t in tor], "loop and batched return the same pairs": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=sorted(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoints_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_keypoints.py measures the device path: it needs a GPU"
    assert args.rounds >= 7 and args.inner >= 1, "at least 7 rounds"
    for name in args.shapes:
        line = json.dumps(run(name, SHAPES[name], args.rounds, args.inner))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
