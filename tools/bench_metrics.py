"""Benchmark of the on-device pose scoring (roma_amd.pose_error / ErrorLog, csrc/metrics.hip) against the route it replaces, on the
shape of the MegaDepth-1500 pose benchmark with its five repeats batched eight pairs at a time: 188 calls of B = 40 poses, then the
summary over the 7 520 errors.
  A  host    the route before: every call reads R, t, ok back (three copies that synchronise), scores the 40 poses in numpy
             (vectorised - kinder to this leg than the reference's per-pair loop), and at the end runs pose_auc (sort, trapezoid)
             and the accuracy lines in numpy;
  B  device  every call is one roma_amd.pose_error(log=) launch, nothing read back; at the end ErrorLog.pose_summary(), one launch
             and the one read.
Only the scoring tail is timed: the poses are made once and lie on the device, as estimate_pose leaves them; the ground truth is
host numpy in both legs, as a data set yields it.  Both legs run interleaved (A B A B) in one process after a warm-up; each leg is
a host clock around work that ends in a device synchronise (A's last read, B's summary read); median and min - max over --rounds
rounds.  The device is idle between calls here, so A's reads wait for nothing: in a real loop each of them also drains the
matcher's queue, which this tool does not measure.  The two legs' results are compared.  One JSON line, appended to --out
(profiles/metrics_bench.jsonl) and printed.  Reported, not gated.
Usage: python tools/bench_metrics.py [--rounds 9] [--calls 188] [--batch 40]
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
THRESHOLDS = (5.0, 10.0, 20.0)


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def rotations(rng, n, max_angle):
    """n rotations by up to max_angle radians about random axes (Rodrigues)"""
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0.0, max_angle, n) ** 2 / max_angle  # most of them small, as a benchmark's errors are
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    return np.eye(3) + np.sin(ang)[:, None, None] * K + (1.0 - np.cos(ang))[:, None, None] * (K @ K)


def host_pose_errors(R, t, ok, T):
    """numpy, vectorised over the batch: the reference's compute_pose_error, e_pose and the 90-degree fallback"""
    Rg, tg = T[:, :, :3], T[:, :, 3]
    n = np.linalg.norm(t, axis=1) * np.linalg.norm(tg, axis=1)
    e_t = np.rad2deg(np.arccos(np.clip((t * tg).sum(axis=1) / n, -1.0, 1.0)))
    e_t = np.minimum(e_t, 180.0 - e_t)
    e_R = np.rad2deg(np.abs(np.arccos(np.clip(((R * Rg).sum(axis=(1, 2)) - 1.0) / 2.0, -1.0, 1.0))))
    return np.where(ok, np.maximum(e_t, e_R), 90.0)


def host_summary(errors):
    """numpy pose_auc (sort, trapezoid) and the accuracy / mAP lines"""
    e = np.sort(errors)
    recall = np.arange(1, e.size + 1) / e.size
    e, recall = np.r_[0.0, e], np.r_[0.0, recall]
    out = {}
    for thr in THRESHOLDS:
        last = np.searchsorted(e, thr)
        x, y = np.r_[e[:last], thr], np.r_[recall[:last], recall[last - 1]]
        out[f"auc_{int(thr)}"] = float(((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0).sum() / thr)
    acc = [float((errors < thr).mean()) for thr in (5, 10, 15, 20)]
    out.update(map_5=acc[0], map_10=float(np.mean(acc[:2])), map_20=float(np.mean(acc)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=188)
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics.py measures the device path: it needs a GPU"
    assert args.rounds >= 7, "at least 7 rounds"
    import roma_amd
    rng = np.random.default_rng(0)
    C, B = args.calls, args.batch
    n = C * B
    Rg = rotations(rng, n, np.pi)
    tg = rng.standard_normal((n, 3))
    T = np.concatenate([Rg, tg[:, :, None]], axis=2).reshape(C, B, 3, 4)
    R = (Rg @ rotations(rng, n, 0.6)).reshape(C, B, 3, 3)
    t = np.einsum("nij,nj->ni", rotations(rng, n, 0.6), tg).reshape(C, B, 3, 1)
    ok = (rng.random((C, B)) > 0.03)  # a few pairs without a pose
    Rd, td, okd = (torch.from_numpy(x).to(DEV) for x in (R, t, ok))

    def leg_host():
        errors = []
        for c in range(C):
            Rh, th, okh = Rd[c].cpu().numpy(), td[c].cpu().numpy(), okd[c].cpu().numpy()
            errors.append(host_pose_errors(Rh, th[:, :, 0], okh, T[c]))
        return host_summary(np.concatenate(errors))

    def leg_device():
        log = roma_amd.ErrorLog(device=DEV)
        for c in range(C):
            roma_amd.pose_error(Rd[c], td[c], T[c], ok=okd[c], log=log)
        return log.pose_summary()

    for fn in (leg_host, leg_device, leg_host, leg_device):  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    ms = {"host ms": [], "device ms": []}
    for _ in range(args.rounds):
        for key, fn in (("host ms", leg_host), ("device ms", leg_device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    a, b = leg_host(), leg_device()
    res = {"config": "metrics", "calls": C, "batch": B, "errors": n, "rounds": args.rounds, **{k: stats(v) for k, v in ms.items()},
           "host over device": round(float(np.median(ms["host ms"]) / np.median(ms["device ms"])), 2),
           "device faster than host in every round": bool(np.max(ms["device ms"]) < np.min(ms["host ms"])),
           "per call us": {k.split()[0]: round(float(np.median(v)) * 1e3 / C, 1) for k, v in ms.items()},
           "summary": {"host": a, "device": b},
           "worst relative difference": float(max(abs(a[k] - b[k]) / abs(a[k]) for k in a if a[k] != 0))}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
