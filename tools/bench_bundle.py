"""Microbenchmark of the device bundle adjustment (roma_amd.bundle_adjust, csrc/bundle.hip): B = 8 problems of N = 5 000 points
at V = 2 and V = 3 views (the scenes of tools/bundle_scenes.py: relief depth 3 - 5, 0.5 px noise, 10 % gross outliers, threshold
2 px, a fifth of the observations missing at V = 3, the start 2e-3 off in the points and 5e-4 in the poses), and next to it
refine_absolute_pose - the nearest sibling: one camera against held points - on the same B and N (view 1 of the V = 2 problems).

The calls are timed alternately in --rounds rounds of --iters calls each (device events around each block, after a warm-up of
every call), medians over the rounds: other work shares the machine, and a difference is only read against the spread of the
same call.  A workgroup runs one problem, so a call takes as long as its slowest problem: the time per accepted step divides
by the largest number of accepted steps in the batch.  One JSON line per call appended to profiles/bundle_bench.jsonl.
Usage: python tools/bench_bundle.py [--iters 20] [--rounds 9] [--out profiles/bundle_bench.jsonl]
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
from bundle_ref import default_hold  # noqa: E402
from bundle_scenes import scene, start  # noqa: E402

THR = 2.0


def batch(B, V, N, missing):
    """(K [B, V, 3, 3], kpts [B, V, N, 2], start X [B, N, 3], R [B, V, 3, 3], t [B, V, 3]) of B scenes of tools/bundle_scenes.py"""
    out = []
    for b in range(B):
        s = scene(V, N, 100 * V + b, missing=missing, noise_px=0.5, outlier_frac=0.1, thr=THR)
        X, R, t = start(s, 200 * V + b, 2e-3, 5e-4)
        out.append((s["K"], s["kpts"], X, R, t))
    return tuple(np.stack(v) for v in zip(*out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--N", type=int, default=5000)
    ap.add_argument("--max-steps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bundle: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import bundle_adjust, refine_absolute_pose
    dev = "cuda:0"
    calls, steps = {}, {}
    for V, missing in ((2, 0.0), (3, 0.2)):
        K, kp, X, R, t = batch(args.B, V, args.N, missing)
        a = dict(X=torch.tensor(X, device=dev), kp=torch.tensor(kp, dtype=torch.float32, device=dev), K=torch.tensor(K, device=dev),
                 R=torch.tensor(R, device=dev), t=torch.tensor(t, device=dev),
                 hold=torch.tensor(np.stack([default_hold(ti) for ti in t]), dtype=torch.uint8, device=dev))
        calls[f"bundle_adjust V={V}"] = lambda a=a: bundle_adjust(a["X"], a["kp"], a["K"], a["R"], a["t"], THR, args.max_steps, hold=a["hold"])
        steps[f"bundle_adjust V={V}"] = lambda out: (out.info[:, 0], out.info[:, 1], out.cost)
        if V == 2:
            b = dict(R=a["R"][:, 1].contiguous(), t=a["t"][:, 1, :, None].contiguous(), X=a["X"].float(), kp=a["kp"][:, 1].contiguous(), K=a["K"][:, 1])
            calls["refine_absolute_pose"] = lambda b=b: refine_absolute_pose(b["R"], b["t"], b["X"], b["kp"], b["K"], THR, args.max_steps)
            steps["refine_absolute_pose"] = lambda out: (out[3][:, 0], out[3][:, 1], None)
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.iters)
    lines = []
    for name, fn in calls.items():
        st, ev, cost = steps[name](fn())
        st, ev = st.cpu().numpy(), ev.cpu().numpy()
        med = float(np.median(ms[name]))
        res = {"call": name, "B": args.B, "N": args.N, "threshold_px": THR, "max_steps": args.max_steps, "iters": args.iters,
               "rounds": args.rounds, "ms_per_call_median": round(med, 4), "ms_per_call_min": round(float(np.min(ms[name])), 4),
               "ms_per_call_max": round(float(np.max(ms[name])), 4), "accepted_steps": st.tolist(), "cost_evaluations": ev.tolist(),
               "ms_per_accepted_step": round(med / max(int(st.max()), 1), 4), "ms_per_cost_evaluation": round(med / max(int(ev.max()), 1), 4),
               "device": torch.cuda.get_device_name(0)}
        if cost is not None:
            res["cost_start_end"] = [[float(f"{v:.6e}") for v in row] for row in cost.cpu().numpy()]
        print(json.dumps(res), flush=True)
        lines.append(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
