"""Microbenchmark of the device relative-pose path (roma_amd.estimate_pose: csrc/essential.hip) at the settings of the
reference's MegaDepth-1500 benchmark: B = 8 pairs, N = 5 000 matches, threshold 0.5 px / mean focal length, confidence
0.99999, OpenCV's default 1 000 iterations, on the relief scenes of accuracy_harness.synthetic_relief_pair with 0 %, 30 % and
50 % uniform outliers.

Per configuration one JSON line: ms per batched estimate_pose call (device events, after warm-up), rounds executed per pair,
hypothesis-point evaluations per second (hypotheses the score kernel ran x points; a hypothesis carries up to 10 models) and the host numpy path
tools/pose_geometry.estimate_pose on the same pairs, one after the other - a CPU number, for scale only.
--refine adds, after each configuration's line, one line for estimate_pose(..., refine=True) (the Levenberg-Marquardt fit of
csrc/pose_refine.hip after the RANSAC): ms per call, the added ms over the plain call timed next to it, steps and cost
evaluations per pair.  With --parent-lib DIR (a directory holding another build of libroma_hip.so, e.g. the parent commit's)
that build's refined call and its refine_pose alone are timed in the same alternation (--rounds each, the medians), and the
outputs of refine_pose are compared build against build, bit for bit, on the bench batch and on a ragged batch
(bench_geometry.ragged_batch).  Without --refine, --parent-lib adds one line per configuration (bench_geometry.against_parent):
every output of `essential`, of estimate_pose with and without refine, and of estimate_pose_uncalibrated for both methods with
and without refine, on the bench batch and on the pipeline's ragged batch, build against build, both timed alternately.
Usage: python tools/bench_pose.py [--iters 20] [--no-cpu] [--rounds 7] [--parent-lib DIR] [--refine]
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
from bench_geometry import (pipeline_counts, _other_build, _stats, _using, against_parent, outputs_equal, ragged_batch,  # noqa: E402
                            relief_batch, within_spread)
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


def pose_calls(a, b, K, method, fns=("essential", "estimate_pose", "estimate_pose_uncalibrated")):
    """{name: call} of the relative-pose entry points for `method` on the bench batch and on the pipeline's ragged batch"""
    from roma_amd import geometry as g
    thr = 0.5 / float(np.mean([K[0, 0], K[1, 1]]))
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    ra, rb, counts = ragged_batch(a, b, 5, counts=pipeline_counts(5))
    ess = g.essential if method == "ransac" else g.essential_magsac
    calls = {}
    for tag, x, y, kw in (("", da, db, {}), (" ragged", ra, rb, {"counts": counts})):
        if "essential" in fns:
            calls[ess.__name__ + tag] = lambda x=x, y=y, kw=kw: ess(x, y, K, 0.99999, 0.5, 1000 if not tag else 600, seed=seeds, **kw)
        for refine in (False, True):
            for fn, t, iters in ((g.estimate_pose, thr, 1000), (g.estimate_pose_uncalibrated, 0.5, 10000)):
                if fn.__name__ in fns:
                    calls[f"{fn.__name__} {method}{' refine=True' if refine else ''}{tag}"] = (
                        lambda fn=fn, t=t, iters=iters, refine=refine, x=x, y=y, kw=kw:
                        fn(x, y, K, K, t, 0.99999, iters if not tag else 600, seed=seeds, refine=refine, method=method, **kw))
    return calls


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def run_refined(name, a, b, K, iters, rounds, parent):
    """the refined leg: the plain call, the refined call and refine_pose alone - and the parent build's refined call and
    refine_pose alone if given - timed alternately in rounds (the medians), and the fit's own counters"""
    from roma_amd.geometry import estimate_pose, refine_pose
    thr = 0.5 / float(np.mean([K[0, 0], K[1, 1]]))
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    plain = lambda: estimate_pose(da, db, K, K, thr, 0.99999, 1000, seed=seeds)  # noqa: E731
    fitted = lambda: estimate_pose(da, db, K, K, thr, 0.99999, 1000, seed=seeds, refine=True)  # noqa: E731
    R, t, mask, ok = plain()
    alone = lambda: refine_pose(R, t, da, db, K, K, thr, valid=ok)  # noqa: E731
    legs = {"plain ms": (None, plain), "this refine=True ms": (None, fitted), "this refine_pose alone ms": (None, alone)}
    if parent is not None:
        legs = {"parent refine=True ms": (parent, fitted), "parent refine_pose alone ms": (parent, alone), **legs}
    for lib, fn in legs.values():
        with _using(lib):
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (lib, fn) in legs.items():
            with _using(lib):
                ms[k].append(_timed(fn, iters)[0])
    info = alone()[3].cpu().numpy()
    res = {"config": name + " refine=True", "B": int(a.shape[0]), "N": int(a.shape[1]), "threshold": thr, "max_steps": 25,
           "ms_per_call": round(float(np.median(ms["this refine=True ms"])), 4), "ms_per_plain_call": round(float(np.median(ms["plain ms"])), 4),
           "added_ms": round(float(np.median(ms["this refine=True ms"]) - np.median(ms["plain ms"])), 4),
           "refine_pose_alone_ms": round(float(np.median(ms["this refine_pose alone ms"])), 4),
           "rounds": rounds, "iters_per_round": iters, **{k: _stats(v) for k, v in ms.items()},
           "steps_per_pair": info[:, 0].tolist(), "cost_evals_per_pair": info[:, 1].tolist(), "active_rows_per_pair": info[:, 2].tolist()}
    if parent is not None:
        names = ("R", "t", "mask", "info")
        res["refined outputs equal the parent's"] = outputs_equal(parent, alone, names)
        # every row of the ragged batch starts from pair 0's pose at its full count
        ra, rb, counts = ragged_batch(a, b, 5)
        R0, t0, _ = estimate_pose(ra[0], rb[0], K, K, thr, 0.99999, 1000, seed=1)
        res["ragged refined outputs equal the parent's"] = outputs_equal(
            parent, lambda: refine_pose(R0.expand(8, 3, 3).contiguous(), t0.expand(8, 3, 1).contiguous(), ra, rb, K, K, thr, counts=counts),
            names)
        for leg in ("refine=True", "refine_pose alone"):
            res[f"{leg} within the parent's spread"] = within_spread(ms[f"this {leg} ms"], ms[f"parent {leg} ms"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host reference timing")
    ap.add_argument("--refine", action="store_true", help="add the estimate_pose(..., refine=True) leg")
    ap.add_argument("--rounds", type=int, default=7, help="--refine, --parent-lib: alternating rounds per leg")
    ap.add_argument("--parent-lib", default=None, help="directory of another build of libroma_hip.so to time next to this one and compare outputs with")
    args = ap.parse_args()
    parent = _other_build(args.parent_lib) if args.parent_lib else None
    assert torch.cuda.is_available(), "bench_pose.py measures the device path: it needs a GPU"
    K = synthetic_relief_pair(480, 640, seed=0)["K1"]
    for frac in (0.0, 0.3, 0.5):
        a, b = relief_batch(8, 5000, frac)
        run(f"estimate_pose megadepth outliers={frac}", a, b, K, args.iters, not args.no_cpu)
        if args.refine:
            run_refined(f"estimate_pose megadepth outliers={frac}", a, b, K, args.iters, args.rounds, parent)
        elif parent is not None:
            calls = {**pose_calls(a, b, K, "ransac"), **pose_calls(a, b, K, "magsac", ("estimate_pose_uncalibrated",))}
            print(json.dumps({"config": f"estimate_pose megadepth outliers={frac} against the parent build", "rounds": args.rounds,
                              "iters_per_round": args.iters, **against_parent(parent, calls, args.iters, args.rounds)}), flush=True)


if __name__ == "__main__":
    main()
