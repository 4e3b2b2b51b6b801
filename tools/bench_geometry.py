"""Microbenchmark of the device RANSAC (roma_amd.geometry, csrc/geometry.hip) at the settings of the reference's consumers:

  * find_fundamental at B = 8, N = 10 000, threshold 0.2 px, confidence 0.999999, max_iters 10 000 (demo_fundamental), on the
    relief scene of accuracy_harness.synthetic_relief_pair with 0 % and 30 % uniform outliers;
  * find_homography at B = 8, N = 5 000 with the HPatches benchmark's settings (threshold 3 min(w, h) / 480 at 864^2,
    confidence 0.99999, OpenCV's default 2 000 iterations), 0.5 px noise and 30 % outliers.

Each configuration runs twice at the same settings: plain RANSAC + LO (`ransac`, the default of find_*) and MAGSAC++ scoring
with IRLS local optimisation (`magsac`, method="magsac").  Per leg one JSON line: ms per batched call (device events, after
warm-up), model-point evaluations per second (the hypotheses the score kernel ran x models per hypothesis x points), rounds
executed per pair, and the same work through tools/geometry_ref.py / tools/magsac_ref.py on the host (numpy f64, one pair after
the other) - a CPU number, for scale only.
Usage: python tools/bench_geometry.py [--iters 20] [--no-cpu] [--method ransac|magsac|both]
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
import geometry_ref as gr  # noqa: E402
import magsac_ref as mr  # noqa: E402
from accuracy_harness import synthetic_relief_pair  # noqa: E402


def relief_batch(B, N, outlier_frac, seed=0, h=480, w=640):
    a, b = np.zeros((B, N, 2)), np.zeros((B, N, 2))
    for i in range(B):
        d = synthetic_relief_pair(h, w, seed=seed + i)
        m = d["gt_matches"].double().numpy().reshape(-1, 4)
        vis = np.nonzero(d["gt_certainty"].numpy().reshape(-1) > 0)[0]
        rng = np.random.default_rng(seed + i)
        sel = rng.choice(vis, N, replace=False)
        a[i] = np.stack([(m[sel, 0] + 1) * w / 2, (m[sel, 1] + 1) * h / 2], 1)
        b[i] = np.stack([(m[sel, 2] + 1) * w / 2, (m[sel, 3] + 1) * h / 2], 1)
        out = rng.random(N) < outlier_frac
        b[i, out] = rng.uniform([0, 0], [w, h], (out.sum(), 2))
    return a, b


def homography_batch(B, N, outlier_frac, seed=0, size=864):
    a, b = np.zeros((B, N, 2)), np.zeros((B, N, 2))
    for i in range(B):
        rng = np.random.default_rng(100 + seed + i)
        H = np.eye(3) + np.array([[0.1, 0.05, 20], [-0.05, 0.1, 15], [1e-4, 1e-4, 0]]) * rng.uniform(-1, 1, (3, 3))
        a[i] = rng.uniform(0, size, (N, 2))
        q = np.c_[a[i], np.ones(N)] @ H.T
        b[i] = q[:, :2] / q[:, 2:] + 0.5 * rng.normal(size=(N, 2))
        out = rng.random(N) < outlier_frac
        b[i, out] = rng.uniform(0, size, (out.sum(), 2))
    return a, b


def run(name, model, a, b, thr, conf, max_iters, iters, cpu, method="ransac"):
    from roma_amd.geometry import magsac, ransac
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    fn = ransac if method == "ransac" else magsac

    def call():
        return fn(model, da, db, thr, conf, max_iters, seed=seeds)[:4]
    for _ in range(3):
        M, mask, ok, info = call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        M, mask, ok, info = call()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    info = info.cpu().numpy()
    roots = gr.MAX_ROOTS if model == gr.FUNDAMENTAL else 1
    evals = float(info[:, 0].sum()) * gr.ROUND * roots * a.shape[1]
    res = {"config": name, "method": method, "B": int(a.shape[0]), "N": int(a.shape[1]), "threshold": thr, "confidence": conf, "max_iters": max_iters,
           "ms_per_call": round(ms, 4), "model_point_evals_per_s": evals / (ms * 1e-3), "rounds_per_pair": info[:, 0].tolist(),
           "inliers_per_pair": info[:, 4].tolist(), "ok": ok.cpu().tolist()}
    if cpu:
        t = time.perf_counter()
        rounds = []
        for i in range(len(a)):
            pa, pb = a[i].astype(np.float32).astype(np.float64), b[i].astype(np.float32).astype(np.float64)
            if method == "ransac":
                r = gr.ransac(model, pa, pb, thr, conf, max_iters, i + 1, True)
            else:
                r = mr.magsac(model, pa, pb, thr, conf, max_iters, i + 1)
            rounds.append(r["rounds"])
        res["cpu_numpy_reference_ms_per_call"] = round((time.perf_counter() - t) * 1e3, 1)
        res["cpu_reference_rounds_per_pair"] = rounds
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host reference timing")
    ap.add_argument("--method", choices=("ransac", "magsac", "both"), default="both")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_geometry.py measures the device path: it needs a GPU"
    methods = ("ransac", "magsac") if args.method == "both" else (args.method,)
    B = 8
    for frac in (0.0, 0.3):
        a, b = relief_batch(B, 10000, frac)
        for m in methods:
            run(f"find_fundamental demo_fundamental outliers={frac}", gr.FUNDAMENTAL, a, b, 0.2, 0.999999, 10000, args.iters,
                not args.no_cpu, m)
    a, b = homography_batch(B, 5000, 0.3)
    for m in methods:
        run("find_homography hpatches outliers=0.3", gr.HOMOGRAPHY, a, b, 3 * 864 / 480, 0.99999, 2000, args.iters, not args.no_cpu,
            m)


if __name__ == "__main__":
    main()
