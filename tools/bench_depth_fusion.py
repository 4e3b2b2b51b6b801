"""Microbenchmark of dense depth fusion (roma_amd.fuse_depth_maps; csrc/depth_fusion.hip), after the method of
tools/bench_set_keypoints.py: the calls are timed alternately in --rounds rounds of --iters calls each, device events around each
block after a warm-up of every call, medians over the rounds.

  fuse_depth_maps    V = 8, all 28 symmetric pairs, grid 864 x 864, B = 1; and V = 4 (6 pairs), B = 8.  The hypotheses are made on
                     the device: a tilted plane seen by cameras in a row, 0.5 % depth noise, 10 % outlier slots, 5 % flagged
  torch yardstick    the same device, the vote and the weighted mean only (float64 tensors, the operator's order of operations):
                     no cross-view check, no duplicates, no cloud.  It is checked to give the operator's `depth`
  kernels            the time of each of the five kernels, from the library's per-launch events in a pass of their own; for the
                     select kernel the bytes it must read (depth 4, flag 1, certainty 4 per slot) and the bytes its loads fetch
                     (the 12-byte stride of the points brings all three floats in) against its time

One JSON line per call appended to profiles/depth_fusion_bench.jsonl, the per-kernel figures to
profiles/depth_fusion_bench_kernel_stats.csv.
Usage: python tools/bench_depth_fusion.py [--iters 20] [--rounds 9] [--out profiles/depth_fusion_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 864
REL = 0.01


def problem(V, B, dev):
    """device tensors of B problems: points [B, P, H, 2W, 3], flags, certainty, and the host pairs, cameras and poses"""
    pairs = [(a, b) for a in range(V) for b in range(a + 1, V)]
    g = torch.Generator(device=dev).manual_seed(V * 100 + B)
    K = np.array([[float(W), 0.0, W / 2.0 + 0.13], [0.0, float(W), H / 2.0 - 0.21], [0.0, 0.0, 1.0]])
    R = np.stack([np.eye(3)] * V)
    t = np.array([[-0.05 * v, 0.0, 0.0] for v in range(V)])
    c, r = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float64) + 0.5, torch.arange(H, device=dev, dtype=torch.float64) + 0.5, indexing="xy")
    x0, x1 = (c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1]
    # the plane z_w = 5 + 0.4 x_w + 0.2 y_w seen from (0.05 v, 0, 0): z (1 - 0.4 x0 - 0.2 x1) = 5 + 0.4 * 0.05 v
    truth = [((5.0 + 0.02 * v) / (1.0 - 0.4 * x0 - 0.2 * x1)).to(torch.float32) for v in range(V)]
    P = len(pairs)
    points = torch.empty((B, P, H, 2 * W, 3), device=dev, dtype=torch.float32)
    for p, (i, j) in enumerate(pairs):
        points[:, p, :, :W, 2], points[:, p, :, W:, 2] = truth[i], truth[j]
    z = points[..., 2]
    z *= 1.0 + 0.005 * torch.randn(z.shape, device=dev, generator=g)
    out = torch.rand(z.shape, device=dev, generator=g) < 0.10
    z *= torch.where(out, 1.5, 1.0)
    points[..., 0], points[..., 1] = 0.0, 0.0
    flags = (torch.rand(z.shape, device=dev, generator=g) < 0.05).to(torch.uint8) * 4
    cert = torch.where(torch.rand(z.shape, device=dev, generator=g) < 0.5, 1.0, 0.6).to(torch.float32)
    f64 = lambda x: torch.as_tensor(np.stack([x] * B), device=dev)  # noqa: E731
    return points, flags, cert, pairs, f64(np.stack([K] * V)), f64(R), f64(t)


def torch_route(points, flags, cert, pairs, V, min_support=2):
    """the vote and the weighted mean only, view by view, in the operator's order of operations"""
    depth = []
    for v in range(V):
        slots = [(p, h) for p, pr in enumerate(pairs) for h in range(2) if pr[h] == v]
        Z = [points[:, p, :, h * W:(h + 1) * W, 2] for p, h in slots]
        U = [(flags[:, p, :, h * W:(h + 1) * W] == 0) & torch.isfinite(z) & (z > 0) & (cert[:, p, :, h * W:(h + 1) * W] > 0) for (p, h), z in zip(slots, Z)]
        Wt = [torch.where(u, cert[:, p, :, h * W:(h + 1) * W], 0.0).double() for (p, h), u in zip(slots, U)]
        Z = [torch.where(u, z, 0.0).double() for u, z in zip(U, Z)]
        WZ = [w * z for w, z in zip(Wt, Z)]
        best_n = torch.zeros_like(Z[0], dtype=torch.int32)
        best_s, best_m = torch.zeros_like(Z[0]), torch.zeros_like(Z[0])
        for k in range(len(slots)):
            nk = torch.zeros_like(best_n)
            sk, mk = torch.zeros_like(Z[0]), torch.zeros_like(Z[0])
            for l in range(len(slots)):
                sup = U[l] & ((Z[l] - Z[k]).abs() <= REL * torch.minimum(Z[l], Z[k]))
                nk = nk + sup
                sk = sk + torch.where(sup, Wt[l], 0.0)
                mk = mk + torch.where(sup, WZ[l], 0.0)
            better = U[k] & ((nk > best_n) | ((nk == best_n) & (sk > best_s)))
            best_n, best_s, best_m = torch.where(better, nk, best_n), torch.where(better, sk, best_s), torch.where(better, mk, best_m)
        depth.append(torch.where(best_n >= min_support, best_m / best_s, float("nan")).float())
    return torch.stack(depth, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_fusion_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_fusion: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import _lib, fuse_depth_maps
    dev = "cuda:0"
    lib = _lib.load()
    lines, stage_rows = [], []
    for V, B in ((8, 1), (4, 8)):
        points, flags, cert, pairs, K, R, t = problem(V, B, dev)
        # max_points: a quarter of the pixels - more than the cloud that is left after the duplicates are dropped
        fuse = lambda: fuse_depth_maps(points, flags, cert, pairs, K, R, t, symmetric=True, rel_thresh=REL, max_points=V * H * W // 4)  # noqa: E731
        yard = lambda: torch_route(points, flags, cert, pairs, V)  # noqa: E731
        calls = {f"fuse_depth_maps V={V} B={B}": fuse, f"torch vote + weighted mean V={V} B={B}": yard}
        for fn in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        out, ref = fuse(), yard()
        if not torch.equal(torch.nan_to_num(out.depth, nan=-1.0), torch.nan_to_num(ref, nan=-1.0)):
            raise SystemExit("bench_depth_fusion: the torch yardstick does not give the operator's depth")
        del ref
        ms = {name: [] for name in calls}
        for _ in range(args.rounds):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters if name.startswith("fuse") else max(1, args.iters // 10)):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / (args.iters if name.startswith("fuse") else max(1, args.iters // 10)))
        # the kernels, in a pass of their own
        lib.roma_profile_enable(1)
        for _ in range(args.iters):
            fuse()
        torch.cuda.synchronize()
        n = lib.roma_profile_report(None, 0)
        buf = C.create_string_buffer(int(n))
        lib.roma_profile_report(buf, n)
        lib.roma_profile_enable(0)
        stages = {k: round(v["total_ms"] / v["calls"], 4) for k, v in json.loads(buf.value.decode()).items() if k.startswith("fuse_")}
        slots = 2 * len(pairs)  # summed over the views
        must = B * H * W * slots * 9.0
        fetched = B * H * W * slots * 17.0
        sel = stages.get("fuse_select_kernel", float("nan"))
        for name in ms:
            res = {"call": name, "iters": args.iters, "rounds": args.rounds, "ms_per_call_median": round(float(np.median(ms[name])), 4),
                   "ms_per_call_min": round(float(np.min(ms[name])), 4), "ms_per_call_max": round(float(np.max(ms[name])), 4),
                   "device": torch.cuda.get_device_name(0)}
            if name.startswith("fuse"):
                res.update({"B": B, "V": V, "P": len(pairs), "grid": [H, W], "stats": out.stats.reshape(-1, 8)[0].cpu().tolist(),
                            "total": out.total.reshape(-1)[0].item(), "stage_ms": stages,
                            "select_must_read_GB": round(must / 1e9, 4), "select_must_read_GBps": round(must / 1e6 / sel, 1),
                            "select_fetched_GB": round(fetched / 1e9, 4), "select_fetched_GBps": round(fetched / 1e6 / sel, 1),
                            "torch_yardstick_over_this": round(float(np.median(ms[f"torch vote + weighted mean V={V} B={B}"]) / np.median(ms[name])), 2)})
            print(json.dumps(res), flush=True)
            lines.append(res)
        stage_rows += [(V, B, k, v) for k, v in stages.items()]
        del points, flags, cert, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")
    with open(os.path.splitext(args.out)[0] + "_kernel_stats.csv", "w") as f:
        f.write("V,B,kernel,ms_per_call\n")
        for row in stage_rows:
            f.write(",".join(str(x) for x in row) + "\n")


if __name__ == "__main__":
    main()
