"""Microbenchmark of the device relative-pose path (roma_amd.estimate_pose: csrc/essential.hip) at the settings of the
reference's MegaDepth-1500 benchmark: B = 8 pairs, N = 5 000 matches, threshold 0.5 px / mean focal length, confidence
0.99999, OpenCV's default 1 000 iterations, on the relief scenes of accuracy_harness.synthetic_relief_pair with 0 %, 30 % and
50 % uniform outliers.

Per configuration one JSON line: ms per batched estimate_pose call (device events, after warm-up), rounds executed per pair,
hypothesis-point evaluations per second (hypotheses the score kernel ran x points; a hypothesis carries up to 10 models) and the host numpy path
tools/pose_geometry.estimate_pose on the same pairs, one after the other - a CPU number, for scale only.
--refine adds, after each configuration's line, one line for estimate_pose(..., refine=True) (the Levenberg-Marquardt fit of
csrc/pose_refine.hip after the RANSAC): ms per call, the added ms over the plain call timed next to it, steps and cost
evaluations per pair.
Usage: python tools/bench_pose.py [--iters 20] [--no-cpu] [--refine]
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
import pose_geometry as pg  # noqa: E402
from bench_geometry import relief_batch  # noqa: E402
from accuracy_harness import synthetic_relief_pair  # noqa: E402


def run(name, a, b, K, iters, cpu):
    from roma_amd.geometry import essential, estimate_pose
    thr = 0.5 / float(np.mean([K[0, 0], K[1, 1]]))
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    for _ in range(3):
        R, t, mask, ok = estimate_pose(da, db, K, K, thr, 0.99999, 1000, seed=seeds)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        R, t, mask, ok = estimate_pose(da, db, K, K, thr, 0.99999, 1000, seed=seeds)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    Ki = torch.linalg.inv(torch.tensor(K[:2, :2], device="cuda:0"))
    x0 = (da.double() - torch.tensor(K[:2, 2], device="cuda:0")) @ Ki.T
    x1 = (db.double() - torch.tensor(K[:2, 2], device="cuda:0")) @ Ki.T
    _, _, _, info = essential(x0, x1, None, 0.99999, thr, 1000, seed=seeds)
    info = info.cpu().numpy()
    res = {"config": name, "B": int(a.shape[0]), "N": int(a.shape[1]), "threshold": thr, "confidence": 0.99999, "max_iters": 1000,
           "ms_per_call": round(ms, 4), "rounds_per_pair": info[:, 0].tolist(), "inliers_per_pair": info[:, 3].tolist(),
           "ok": ok.cpu().tolist()}
    evals = float(info[:, 0].sum()) * 256 * a.shape[1]  # hypotheses scored x points (each hypothesis has up to 10 models)
    res["hypothesis_point_evals_per_s"] = evals / (ms * 1e-3)
    if cpu:
        t0 = time.perf_counter()
        for i in range(len(a)):
            pg.estimate_pose(a[i], b[i], K, K, thr, 0.99999, rng=np.random.default_rng(i))
        res["cpu_numpy_pose_geometry_ms_per_call"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res), flush=True)
    return res


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def run_refined(name, a, b, K, iters):
    """the refined leg: plain and refined calls timed alternately (three rounds each, the medians), and the fit's own counters"""
    from roma_amd.geometry import estimate_pose, refine_pose
    thr = 0.5 / float(np.mean([K[0, 0], K[1, 1]]))
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    plain = lambda: estimate_pose(da, db, K, K, thr, 0.99999, 1000, seed=seeds)  # noqa: E731
    fitted = lambda: estimate_pose(da, db, K, K, thr, 0.99999, 1000, seed=seeds, refine=True)  # noqa: E731
    for _ in range(3):
        plain()
        fitted()
    torch.cuda.synchronize()
    ms_p, ms_r = [], []
    for _ in range(3):
        ms_p.append(_timed(plain, iters)[0])
        ms_r.append(_timed(fitted, iters)[0])
    R, t, mask, ok = plain()
    ms_fit, (_, _, _, info) = _timed(lambda: refine_pose(R, t, da, db, K, K, thr, valid=ok), iters)
    info = info.cpu().numpy()
    res = {"config": name + " refine=True", "B": int(a.shape[0]), "N": int(a.shape[1]), "threshold": thr, "max_steps": 25,
           "ms_per_call": round(float(np.median(ms_r)), 4), "ms_per_plain_call": round(float(np.median(ms_p)), 4),
           "added_ms": round(float(np.median(ms_r) - np.median(ms_p)), 4), "refine_pose_alone_ms": round(ms_fit, 4),
           "steps_per_pair": info[:, 0].tolist(), "cost_evals_per_pair": info[:, 1].tolist(), "active_rows_per_pair": info[:, 2].tolist()}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host reference timing")
    ap.add_argument("--refine", action="store_true", help="add the estimate_pose(..., refine=True) leg")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pose.py measures the device path: it needs a GPU"
    K = synthetic_relief_pair(480, 640, seed=0)["K1"]
    for frac in (0.0, 0.3, 0.5):
        a, b = relief_batch(8, 5000, frac)
        run(f"estimate_pose megadepth outliers={frac}", a, b, K, args.iters, not args.no_cpu)
        if args.refine:
            run_refined(f"estimate_pose megadepth outliers={frac}", a, b, K, args.iters)


if __name__ == "__main__":
    main()
