"""Microbenchmark of the device absolute pose (roma_amd.absolute_pose, csrc/absolute_pose.hip): estimate_absolute_pose at B = 8,
N = 5 000 on relief scenes (the K, R, t of accuracy_harness.synthetic_relief_pair, relief depth 3 - 5, 0.5 px noise, 30 %
outliers, threshold 1 px), with refine off and on, and next to it estimate_pose(refine=True) - five-point RANSAC, recover_pose,
Sampson LM: the nearest sibling - on the same B, N and max_iters with the same points seen from camera A.

The three calls are timed alternately in --rounds rounds of --iters calls each (device events around each block, after a
warm-up of every call), medians over the rounds: other work shares the machine, and a difference is only read against the
spread of the same call.  One JSON line per call - ms per batched call (median, min, max over the rounds), rounds executed per
pair, inliers, the pose error against the scene - appended to profiles/absolute_pose_bench.jsonl.
Usage: python tools/bench_absolute_pose.py [--iters 20] [--rounds 7] [--max-iters 1000] [--out profiles/absolute_pose_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from accuracy_harness import synthetic_relief_pair  # noqa: E402

H, W, THR = 480, 640, 1.0


def relief_batch(B, N, outlier_frac=0.3, noise=0.5, seed=0):
    """(K [B, 3, 3], R, t, X [B, N, 3] in camera A's frame, kpts_A, kpts_B [B, N, 2])"""
    Ks, Rs, ts, Xs, kas, kbs = [], [], [], [], [], []
    for i in range(B):
        d = synthetic_relief_pair(H, W, seed=seed + i)
        K, T = d["K1"], d["T_1to2"]
        U, _, Vt = np.linalg.svd(T[:, :3])
        R, t = U @ Vt, T[:, 3]
        rng = np.random.default_rng(seed + i)
        ph = rng.uniform(0, 6, 2)
        pa = rng.uniform([0, 0], [W, H], (N, 2))
        z = 4.0 + 0.6 * np.sin(pa[:, 0] / W * 5.0 + ph[0]) + 0.4 * np.cos(pa[:, 1] / H * 4.0 + ph[1])
        X = np.c_[(pa[:, 0] - K[0, 2]) / K[0, 0], (pa[:, 1] - K[1, 2]) / K[1, 1], np.ones(N)] * z[:, None]
        q = X @ R.T + t
        pb = np.stack([K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2], K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]], 1)
        pb += noise * rng.normal(size=pb.shape)
        out = rng.random(N) < outlier_frac
        pb[out] = rng.uniform([0, 0], [W, H], (int(out.sum()), 2))
        for lst, v in zip((Ks, Rs, ts, Xs, kas, kbs), (K, R, t, X, pa, pb)):
            lst.append(v)
    return tuple(np.stack(v) for v in (Ks, Rs, ts, Xs, kas, kbs))


def rot_err_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.einsum("bij,bij->b", Ra, Rb) - 1) / 2, -1, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--N", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absolute_pose_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_absolute_pose: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import estimate_absolute_pose, estimate_pose
    from roma_amd.absolute_pose import absolute_pose
    dev = "cuda:0"
    K, R, t, X, ka, kb = relief_batch(args.B, args.N)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)  # noqa: E731
    Kd, Xd, kad, kbd = torch.tensor(K, device=dev), f32(X), f32(ka), f32(kb)
    seeds = torch.arange(args.B, dtype=torch.int64, device=dev) + 1
    thr_n = THR / float(K[0, 0, 0])
    calls = {
        "estimate_absolute_pose refine=False": lambda: estimate_absolute_pose(Xd, kbd, Kd, THR, 0.9999, args.max_iters, seed=seeds, refine=False),
        "estimate_absolute_pose refine=True": lambda: estimate_absolute_pose(Xd, kbd, Kd, THR, 0.9999, args.max_iters, seed=seeds, refine=True),
        "estimate_pose refine=True": lambda: estimate_pose(kad, kbd, Kd, Kd, thr_n, 0.9999, args.max_iters, seed=seeds, refine=True),
    }
    for fn in calls.values():  # every shape the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.iters)
    info = absolute_pose(Xd, kbd, Kd, THR, 0.9999, args.max_iters, seed=seeds)[4].cpu().numpy()
    lines = []
    for name, fn in calls.items():
        Rd, td, mask, ok = (o.cpu().numpy() for o in fn())
        tt = t / np.linalg.norm(t, axis=1, keepdims=True) if name.startswith("estimate_pose") else t
        res = {"call": name, "B": args.B, "N": args.N, "max_iters": args.max_iters, "threshold_px": THR, "iters": args.iters,
               "rounds": args.rounds, "ms_per_call_median": round(float(np.median(ms[name])), 4),
               "ms_per_call_min": round(float(np.min(ms[name])), 4), "ms_per_call_max": round(float(np.max(ms[name])), 4),
               "ok": ok.tolist(), "inliers_per_pair": mask.sum(axis=1).tolist(),
               "rotation_error_deg_median": float(np.median(rot_err_deg(Rd, R))),
               "translation_error_median": float(np.median(np.linalg.norm(td[:, :, 0] - tt, axis=1))),
               "device": torch.cuda.get_device_name(0)}
        if name.startswith("estimate_absolute"):
            res["ransac_rounds_per_pair"] = info[:, 0].tolist()
        print(json.dumps(res), flush=True)
        lines.append(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
