"""Microbenchmark of the device registration (roma_amd.registration, csrc/registration.hip):
  * align_points at B = 8 problems of N = 5 000 rows, 30 % outliers, with the refinement off and on;
  * register_depth_maps for one 864 x 864 view at step 4 (46 656 rows);
  * trajectory_error for 8 paths of 8 views;
and, on the align_points problem, two yardsticks written here:
  * "torch svd": the same number of three-point hypotheses (the rounds the device ran x 256 per problem) as batched
    torch.linalg.svd Umeyama on the same device, their inlier masks over all rows, the best one's mask - what one would write
    without this operator;
  * "numpy host": the same in numpy on the host, the read-back of the rows included.
The yardsticks draw their samples with a generator of their own: they do the same amount of work, not the same samples.

The device calls are timed alternately in --rounds rounds of --iters calls each (events on the stream around each block, after a
warm-up of every call), medians over the rounds: other work shares the machine, and a difference is only read against the
spread of the same call.  The host route is timed by the wall clock around a synchronised call.  One JSON line per call,
appended to --out.
Usage: python tools/bench_registration.py [--iters 20] [--rounds 5] [--out profiles/registration_bench.jsonl]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_absolute_pose import relief_batch  # noqa: E402

THR_REL, NOISE_REL = 0.02, 0.15  # threshold over the scale; noise per coordinate over the threshold


def _rotation(g):
    q = g.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def problems(B, N, outlier_frac=0.3, seed=0):
    """(X, Y [B, N, 3] f32, scale [B], R [B, 3, 3], t [B, 3], thr): relief points, dst = s R x + t + noise, an outlier's destination
    uniform in the destination's bounding box.  One scale, so that one threshold serves the batch."""
    X = relief_batch(B, N, seed=seed)[3]
    g = np.random.default_rng(seed)
    s, thr = 1.7, THR_REL * 1.7
    R, t = np.stack([_rotation(g) for _ in range(B)]), g.uniform(-3, 3, (B, 3))
    Y = s * np.einsum("bij,bnj->bni", R, X) + t[:, None]
    lo, hi = Y.min(axis=1, keepdims=True), Y.max(axis=1, keepdims=True)
    Y = Y + NOISE_REL * thr * g.normal(size=Y.shape)
    out = g.random((B, N)) < outlier_frac
    Y = np.where(out[..., None], g.uniform(lo, hi, Y.shape), Y)
    return X.astype(np.float32), Y.astype(np.float32), np.full(B, s), R, t, thr


def torch_svd_route(X, Y, thr, hyps, gen):
    """batched SVD Umeyama over `hyps` three-point samples per problem, masks of all, the best: (s, R, t, mask)"""
    B, N = X.shape[:2]
    idx = torch.randint(0, N, (B, hyps, 3), device=X.device, generator=gen)
    bi = torch.arange(B, device=X.device)[:, None, None]
    x, y = X[bi, idx].double(), Y[bi, idx].double()  # [B, H, 3, 3]
    xb, yb = x.mean(dim=2, keepdim=True), y.mean(dim=2, keepdim=True)
    dx, dy = x - xb, y - yb
    U, D, Vt = torch.linalg.svd(dy.transpose(2, 3) @ dx)
    sg = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    S = torch.ones_like(D)
    S[..., 2] = sg
    R = (U * S[..., None, :]) @ Vt
    s = (D * S).sum(dim=-1) / (dx * dx).sum(dim=(2, 3))
    t = yb[:, :, 0] - s[..., None] * (R @ xb[:, :, 0, :, None])[..., 0]
    A, tf = (s[..., None, None] * R).float(), t.float()
    r2 = ((torch.einsum("bhij,bnj->bhni", A, X) + tf[:, :, None] - Y[:, None]) ** 2).sum(dim=-1)  # [B, H, N]
    inl = r2 < thr * thr
    best = inl.sum(dim=-1).argmax(dim=1)
    pick = torch.arange(B, device=X.device)
    return s[pick, best], R[pick, best], t[pick, best], inl[pick, best]


def numpy_host_route(Xd, Yd, thr, hyps, g):
    """the same on the host, the read-back of the rows included"""
    X, Y = Xd.cpu().numpy(), Yd.cpu().numpy()
    out = []
    for b in range(len(X)):
        idx = g.integers(0, X.shape[1], (hyps, 3))
        x, y = X[b][idx].astype(np.float64), Y[b][idx].astype(np.float64)
        xb, yb = x.mean(axis=1, keepdims=True), y.mean(axis=1, keepdims=True)
        dx, dy = x - xb, y - yb
        U, D, Vt = np.linalg.svd(dy.transpose(0, 2, 1) @ dx)
        S = np.ones_like(D)
        S[:, 2] = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
        R = (U * S[:, None, :]) @ Vt
        s = (D * S).sum(axis=1) / (dx * dx).sum(axis=(1, 2))
        t = yb[:, 0] - s[:, None] * np.einsum("hij,hj->hi", R, xb[:, 0])
        A = (s[:, None, None] * R).astype(np.float32)
        r2 = ((np.einsum("hij,nj->hni", A, X[b]) + t[:, None].astype(np.float32) - Y[b][None]) ** 2).sum(axis=-1)
        inl = r2 < thr * thr
        k = int(inl.sum(axis=1).argmax())
        out.append((s[k], R[k], t[k], inl[k]))
    return out


def depth_problem(H, W, dev):
    """two depth maps of one view in gauges that differ by a similarity (tests/registration_cases.depth_case, without the holes)"""
    g = np.random.default_rng(5)
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1.0]])
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    da = 4.0 + 0.6 * np.sin(xs / W * 5.0 + 1.0) + 0.4 * np.cos(ys / H * 4.0 + 2.0)
    s, R, t = 2.3, _rotation(g), g.uniform(-3, 3, 3)
    Ra, ta = np.eye(3), np.zeros(3)
    Rb, tb = Ra @ R, (Ra @ t + ta) / s
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)  # noqa: E731
    return (torch.tensor(da, dtype=torch.float32, device=dev), torch.tensor(da / s, dtype=torch.float32, device=dev), K, (f64(Ra), f64(ta)),
            (f64(Rb), f64(tb)), (s, R, t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--N", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registration_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_registration: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import align_points, register_depth_maps, trajectory_error
    dev = "cuda:0"
    X, Y, s, R, t, thr = problems(args.B, args.N)
    Xd, Yd = torch.tensor(X, device=dev), torch.tensor(Y, device=dev)
    seeds = torch.arange(args.B, dtype=torch.int64, device=dev) + 1
    first = align_points(Xd, Yd, thr, True, 0.9999, args.max_iters, seed=seeds, refine=False)
    rounds_run = first.info[:, 0].cpu().numpy()
    hyps = int(rounds_run.max()) * 256
    gen = torch.Generator(device=dev).manual_seed(1)
    da, db, K, pose_a, pose_b, dsim = depth_problem(864, 864, dev)
    g = np.random.default_rng(3)
    tR = torch.tensor(np.stack([[_rotation(g) for _ in range(8)] for _ in range(8)]), device=dev)
    tt = torch.tensor(g.uniform(-2, 2, (8, 8, 3)), device=dev)
    gR = tR @ torch.tensor(_rotation(g), device=dev)
    gt = 1.8 * tt + 0.01 * torch.tensor(g.normal(size=(8, 8, 3)), device=dev)
    calls = {
        "align_points refine=False": lambda: align_points(Xd, Yd, thr, True, 0.9999, args.max_iters, seed=seeds, refine=False),
        "align_points refine=True": lambda: align_points(Xd, Yd, thr, True, 0.9999, args.max_iters, seed=seeds, refine=True),
        "torch svd": lambda: torch_svd_route(Xd, Yd, thr, hyps, gen),
        "register_depth_maps 864x864 step=4": lambda: register_depth_maps(da[None], db[None], K, (pose_a[0][None], pose_a[1][None]),
                                                                          (pose_b[0][None], pose_b[1][None]), 1e-3, step=4, seed=seeds[:1]),
        "trajectory_error 8x8": lambda: trajectory_error(tR, tt, gR, gt),
    }
    for fn in calls.values():  # every shape the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    ms["numpy host"] = []
    gh = np.random.default_rng(2)
    for _ in range(args.rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.iters)
        t0 = time.perf_counter()
        host = numpy_host_route(Xd, Yd, thr, hyps, gh)
        ms["numpy host"].append(1e3 * (time.perf_counter() - t0))

    def line(name, **extra):
        res = {"call": name, "iters": args.iters if name != "numpy host" else 1, "rounds": args.rounds,
               "ms_per_call_median": round(float(np.median(ms[name])), 4), "ms_per_call_min": round(float(np.min(ms[name])), 4),
               "ms_per_call_max": round(float(np.max(ms[name])), 4), "device": torch.cuda.get_device_name(0)}
        res.update(extra)
        print(json.dumps(res), flush=True)
        return res

    def errors(sc, Rm, tm):
        sc, Rm, tm = (np.asarray(v, dtype=np.float64) for v in (sc, Rm, tm))
        ang = np.degrees(np.arccos(np.clip((np.einsum("bij,bij->b", Rm, R) - 1) / 2, -1, 1)))
        return {"scale_error_rel_median": float(np.median(np.abs(sc / s - 1))), "rotation_error_deg_median": float(np.median(ang)),
                "translation_error_median": float(np.median(np.linalg.norm(tm - t, axis=1)))}

    shape = {"B": args.B, "N": args.N, "max_iters": args.max_iters, "threshold": thr, "outlier_frac": 0.3}
    lines = []
    for name in ("align_points refine=False", "align_points refine=True"):
        o = calls[name]()
        lines.append(line(name, **shape, ok=o.ok.cpu().tolist(), inliers=o.mask.sum(dim=1).cpu().tolist(), ransac_rounds=rounds_run.tolist(),
                          **errors(o.scale.cpu(), o.R.cpu(), o.t.cpu())))
    o = calls["torch svd"]()
    lines.append(line("torch svd", **shape, hypotheses=hyps, inliers=o[3].sum(dim=1).cpu().tolist(), **errors(o[0].cpu(), o[1].cpu(), o[2].cpu())))
    lines.append(line("numpy host", **shape, hypotheses=hyps, inliers=[int(h[3].sum()) for h in host],
                      **errors([h[0] for h in host], [h[1] for h in host], [h[2] for h in host])))
    o = calls["register_depth_maps 864x864 step=4"]()
    lines.append(line("register_depth_maps 864x864 step=4", rows=int(o.mask.shape[1]), inliers=int(o.mask.sum()), ok=bool(o.ok[0]),
                      scale_error_rel=abs(float(o.scale[0]) / dsim[0] - 1), rotation_error_max=float(np.abs(o.R[0].cpu().numpy() - dsim[1]).max()),
                      translation_error=float(np.linalg.norm(o.t[0].cpu().numpy() - dsim[2]))))
    o = calls["trajectory_error 8x8"]()
    lines.append(line("trajectory_error 8x8", B=8, V=8, ok=o.ok.cpu().tolist(), rmse_median=float(o.rmse.median())))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
