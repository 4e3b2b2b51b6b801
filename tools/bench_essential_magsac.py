"""Microbenchmark of the device relative-pose path with MAGSAC++ scoring and local optimisation (roma_amd.estimate_pose(...,
method="magsac"): csrc/ransac.h MagsacScoring on csrc/essential.hip) next to the plain five-point RANSAC it builds on, at the
settings of tools/bench_pose.py: B = 8 pairs, N = 5 000 matches, threshold 0.5 px / mean focal length, confidence 0.99999,
max_iters 1 000, on the relief scenes with 0 %, 30 % and 50 % uniform outliers and 0.5 px of noise in image B.

Per configuration one JSON line: ms per batched estimate_pose call (device events, after warm-up; the four legs method="ransac"
and method="magsac", each with and without refine=True, timed alternately in --rounds rounds, the medians), rounds and LO steps
per pair, and the median pose error of each leg against the scene's pose.  There is no gate on the time.  --parent-lib DIR (a
directory holding another build of libroma_hip.so, e.g. the parent commit's) adds one line per configuration
(bench_geometry.against_parent): every output of `essential_magsac` and of estimate_pose(method="magsac") with and without
refine, on the bench batch and on the pipeline's ragged batch, build against build, both timed alternately.
Usage: python tools/bench_essential_magsac.py [--iters 20] [--rounds 7] [--parent-lib DIR] > profiles/essential_magsac_bench.jsonl
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
import pose_geometry as pg  # noqa: E402
from accuracy_harness import synthetic_relief_pair  # noqa: E402
from bench_geometry import _other_build, _stats, against_parent, relief_batch  # noqa: E402
from bench_pose import _timed, pose_calls  # noqa: E402

B, N, MAX_ITERS, CONF, NOISE = 8, 5000, 1000, 0.99999, 0.5


def run(name, a, b, K, Ts, iters, rounds):
    from roma_amd.geometry import _normalise_pose_points, essential_magsac, estimate_pose
    thr = 0.5 / float(np.mean([K[0, 0], K[1, 1]]))
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    legs = {f"{method}{' refine=True' if refine else ''}":
            (lambda method=method, refine=refine: estimate_pose(da, db, K, K, thr, CONF, MAX_ITERS, seed=seeds, refine=refine,
                                                                method=method))
            for method in ("ransac", "magsac") for refine in (False, True)}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(_timed(fn, iters)[0])
    Kd = torch.as_tensor(K, device="cuda:0")[None].expand(len(a), 3, 3)
    info = essential_magsac(_normalise_pose_points(da, Kd), _normalise_pose_points(db, Kd), None, CONF, thr, MAX_ITERS,
                            seed=seeds)[3].cpu().numpy()
    res = {"config": name, "B": int(a.shape[0]), "N": int(a.shape[1]), "threshold": thr, "confidence": CONF, "max_iters": MAX_ITERS,
           "lo_iters": 10, "noise_px": NOISE, "rounds": rounds, "iters_per_round": iters,
           "ms_per_call": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, **{k + " ms": _stats(v) for k, v in ms.items()},
           "sampling_rounds_per_pair": info[:, 0].tolist(), "lo_steps_per_pair": info[:, 6].tolist(),
           "inliers_minimal_per_pair": info[:, 3].tolist(), "inliers_final_per_pair": info[:, 4].tolist()}
    err = {}
    for k, fn in legs.items():
        R, t, mask, ok = fn()
        R, t = R.cpu().numpy(), t.cpu().numpy()
        assert ok.all()
        err[k] = round(float(np.median([max(pg.compute_pose_error(Ts[i], R[i], t[i])) for i in range(len(a))])), 4)
    res["median_pose_error_deg"] = err
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds per leg")
    ap.add_argument("--parent-lib", default=None, help="directory of another build of libroma_hip.so to time next to this one and compare outputs with")
    args = ap.parse_args()
    parent = _other_build(args.parent_lib) if args.parent_lib else None
    assert torch.cuda.is_available(), "bench_essential_magsac.py measures the device path: it needs a GPU"
    K = synthetic_relief_pair(480, 640, seed=0)["K1"]
    Ts = [synthetic_relief_pair(480, 640, seed=i)["T_1to2"] for i in range(B)]
    for frac in (0.0, 0.3, 0.5):
        a, b = relief_batch(B, N, frac, noise=NOISE)
        run(f"estimate_pose megadepth outliers={frac} noise={NOISE}", a, b, K, Ts, args.iters, args.rounds)
        if parent is not None:
            calls = pose_calls(a, b, K, "magsac", ("essential", "estimate_pose"))
            print(json.dumps({"config": f"estimate_pose megadepth outliers={frac} noise={NOISE} against the parent build",
                              "rounds": args.rounds, "iters_per_round": args.iters,
                              **against_parent(parent, calls, args.iters, args.rounds)}), flush=True)


if __name__ == "__main__":
    main()
