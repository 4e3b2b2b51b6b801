"""Microbenchmark of the multi-view stage (roma_amd.build_tracks / triangulate_views / reconstruct_views; csrc/tracks.hip,
csrc/triangulate_views.hip), after the method of tools/bench_bundle.py: the calls are timed alternately in --rounds rounds of
--iters calls each, device events around each block after a warm-up of every call, medians over the rounds.

  build_tracks        V = 8, K = 4096, all P = 28 pairs (planted tracks of 2 .. 8 views, 5 % false rows), against the host route:
                      read `inds` back, tools/tracks_ref.py, upload the table (wall clock, one call a round)
  triangulate_views   B = 8, N = 5 000 at V = 3 and V = 8 (tools/bundle_scenes.py: 0.5 px noise, 10 % outliers, threshold 2 px),
                      against a torch route on the same device: the midpoint only, by batched 3 x 3 solves
  reconstruct_views   B = 8, V = 4, N = 5 000, with the time of each stage: the five calls it is composed of are made here, a
                      device event after each, and their result is checked against reconstruct_views' own

One JSON line per call appended to profiles/views_bench.jsonl.
Usage: python tools/bench_views.py [--iters 20] [--rounds 9] [--out profiles/views_bench.jsonl]
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
import tracks_ref  # noqa: E402
from bundle_scenes import scene  # noqa: E402

THR = 2.0
CONF = 0.99999  # reconstruct_views' default


def match_graph(V, K, seed, false_frac=0.05):
    """(pairs [P, 2], inds [P, M, 2] padded with -1, match_counts [P]): 2 K / 3 planted tracks of 2 .. V views, every pair of a track's
    views joined, plus false rows"""
    g = np.random.default_rng(seed)
    pairs = [(a, b) for a in range(V) for b in range(a + 1, V)]
    rows = {p: [] for p in pairs}
    free = [list(g.permutation(K)) for _ in range(V)]
    for k in range(2 * K // 3):
        views = sorted(g.choice(V, 2 + k % (V - 1), replace=False).tolist())
        kp = {v: int(free[v].pop()) for v in views}
        for i, a in enumerate(views):
            for b in views[i + 1:]:
                rows[(a, b)].append((kp[a], kp[b]))
    M = max(len(r) for r in rows.values())
    M += int(false_frac * M) + 1
    inds = np.full((len(pairs), M, 2), -1, dtype=np.int32)
    counts = np.zeros(len(pairs), dtype=np.int32)
    for p, pr in enumerate(pairs):
        r = rows[pr] + [(int(g.integers(0, K)), int(g.integers(0, K))) for _ in range(int(false_frac * len(rows[pr])))]
        inds[p, :len(r)], counts[p] = np.asarray(r, dtype=np.int32)[g.permutation(len(r))], len(r)
    return np.asarray(pairs, dtype=np.int32), inds, counts


def scenes(B, V, N, missing, outliers=0.1):
    out = [scene(V, N, 100 * V + b, missing=missing, noise_px=0.5, outlier_frac=outliers, thr=THR) for b in range(B)]
    return tuple(np.stack([s[k] for s in out]) for k in ("K", "kpts", "R", "t"))


def torch_midpoint(kp, K, R, t):
    """the midpoint of the rays of every finite observation, in torch on the device: [B, N, 3]"""
    x = torch.stack(((kp[..., 0].double() - K[:, :, None, 0, 2]) / K[:, :, None, 0, 0], (kp[..., 1].double() - K[:, :, None, 1, 2]) / K[:, :, None, 1, 1],
                     torch.ones_like(kp[..., 0], dtype=torch.float64)), dim=-1)
    d = torch.einsum("bvji,bvnj->bvni", R, x)
    d = d / d.norm(dim=-1, keepdim=True)
    seen = torch.isfinite(d).all(dim=-1)
    d = torch.where(seen[..., None], d, torch.zeros((), dtype=torch.float64, device=d.device))
    c = -torch.einsum("bvji,bvj->bvi", R, t)
    M = seen[..., None, None] * (torch.eye(3, dtype=torch.float64, device=d.device) - d[..., :, None] * d[..., None, :])
    A = M.sum(dim=1)
    b = torch.einsum("bvnij,bvj->bni", M, c)
    X, _ = torch.linalg.solve_ex(A, b[..., None])
    return X[..., 0]


def reconstruct_stages(x, K, seeds, mark):
    """what reconstruct_views(x, K, 1 / 520, THR, seed=seeds) enqueues for V > 2, every view registered or not, stage by stage;
    mark(name) after each.  Returns (R, t, points)."""
    from roma_amd import bundle_adjust, estimate_absolute_pose, estimate_pose, triangulate_views
    from roma_amd.bundle import default_hold
    B, V, N = x.shape[:3]
    f64 = dict(device=x.device, dtype=torch.float64)
    eye, nan = torch.eye(3, **f64), torch.full((), float("nan"), **f64)
    R1, t1, _, ok = estimate_pose(x[:, 0], x[:, 1], K[:, 0], K[:, 1], 1.0 / 520.0, CONF, 1000, seeds, refine=True)
    mark("estimate_pose")
    view_ok = torch.zeros((B, V), device=x.device, dtype=torch.bool)
    view_ok[:, :2] = ok[:, None]
    Rs, ts = eye.expand(B, V, 3, 3).clone(), torch.zeros((B, V, 3), **f64)
    Rs[:, 1], ts[:, 1] = R1, t1.reshape(B, 3)
    tri = triangulate_views(x, K, Rs, ts, view_valid=view_ok, valid=ok, max_reproj=THR)
    pts = torch.where(tri.valid[..., None], tri.points, nan)
    mark("triangulate_views (seed pair)")
    more = V - 2
    step = torch.arange(1, more + 1, device=x.device, dtype=torch.int64) * 1000003
    Rr, tr, _, okr = estimate_absolute_pose(pts[:, None].expand(B, more, N, 3).reshape(B * more, N, 3), x[:, 2:].reshape(B * more, N, 2),
                                            K[:, 2:].reshape(B * more, 3, 3), THR, conf=CONF, max_iters=1000,
                                            seed=(seeds[:, None] + step).reshape(-1), refine=True)
    view_ok = torch.cat((view_ok[:, :2], okr.reshape(B, more) & ok[:, None]), dim=1)
    Rs = torch.where(view_ok[..., None, None], torch.cat((Rs[:, :2], Rr.reshape(B, more, 3, 3)), dim=1), eye).contiguous()
    ts = torch.where(view_ok[..., None], torch.cat((ts[:, :2], tr.reshape(B, more, 3)), dim=1), torch.zeros((), **f64)).contiguous()
    mark("estimate_absolute_pose")
    tri = triangulate_views(x, K, Rs, ts, view_valid=view_ok, valid=ok, max_reproj=THR)
    pts = torch.where(tri.valid[..., None], tri.points, nan)
    mark("triangulate_views")
    hold = default_hold(ts) | (~view_ok[..., None]).to(torch.uint8)
    seen = torch.where(view_ok[:, :, None, None], x, torch.full((), float("nan"), device=x.device, dtype=torch.float32))
    out = bundle_adjust(pts, seen, K, Rs, ts, THR, hold=hold, valid=ok)
    mark("bundle_adjust")
    return out.R, out.t, out.points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--N", type=int, default=5000)
    ap.add_argument("--K", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_views: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import build_tracks, reconstruct_views, triangulate_views
    dev = "cuda:0"
    calls, host, extra = {}, {}, {}

    V, K = 8, args.K
    pairs, inds, counts = match_graph(V, K, 0)
    x = np.random.default_rng(1).uniform(0, 640, (V, K, 2)).astype(np.float32)
    g = dict(inds=torch.tensor(inds, device=dev), counts=torch.tensor(counts, device=dev), x=torch.tensor(x, device=dev), pairs=[tuple(p) for p in pairs])
    calls["build_tracks"] = lambda: build_tracks(g["inds"], g["pairs"], V, match_counts=g["counts"], kpts=g["x"])

    def host_tracks():
        o = tracks_ref.build(g["inds"].cpu().numpy(), pairs, V, K, g["counts"].cpu().numpy(), None, x)
        return torch.tensor(o["tracks"], device=dev), torch.tensor(o["kpts"], device=dev)

    host["build_tracks host route (read back, tracks_ref, upload)"] = host_tracks
    extra["build_tracks"] = lambda out: {"V": V, "K": K, "P": len(pairs), "M": int(inds.shape[1]), "rows": int(counts.sum()), "tracks": int(out.total),
                                         "info": out.info.cpu().tolist()}

    for Vt, missing in ((3, 0.2), (8, 0.3)):
        Kc, kp, R, t = scenes(args.B, Vt, args.N, missing)
        a = dict(kp=torch.tensor(kp, dtype=torch.float32, device=dev), K=torch.tensor(Kc, device=dev), R=torch.tensor(R, device=dev), t=torch.tensor(t, device=dev))
        calls[f"triangulate_views V={Vt}"] = lambda a=a: triangulate_views(a["kp"], a["K"], a["R"], a["t"], max_reproj=THR)
        calls[f"triangulate_views V={Vt} gn_steps=0 trim=False"] = lambda a=a: triangulate_views(a["kp"], a["K"], a["R"], a["t"], gn_steps=0, trim=False)
        calls[f"torch midpoint V={Vt}"] = lambda a=a: torch_midpoint(a["kp"], a["K"], a["R"], a["t"])
        extra[f"triangulate_views V={Vt}"] = lambda out, Vt=Vt: {"B": args.B, "N": args.N, "V": Vt, "stats": out.stats.cpu().tolist()}

    Kc, kp, _, _ = scenes(args.B, 4, args.N, 0.2, outliers=0.05)
    r = dict(kp=torch.tensor(kp, dtype=torch.float32, device=dev), K=torch.tensor(Kc, device=dev), seeds=torch.arange(3, 3 + args.B, device=dev))
    calls["reconstruct_views V=4"] = lambda: reconstruct_views(r["kp"], r["K"], 1.0 / 520.0, THR, seed=r["seeds"])
    extra["reconstruct_views V=4"] = lambda out: {"B": args.B, "N": args.N, "V": 4, "view_ok": out.view_ok.cpu().tolist(), "info": out.info.cpu().tolist()}

    for fn in calls.values():
        for _ in range(3):
            fn()
    whole, parts = calls["reconstruct_views V=4"](), reconstruct_stages(r["kp"], r["K"], r["seeds"], lambda stage: None)
    if not all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip((whole.R, whole.t, whole.points), parts)):
        raise SystemExit("bench_views: the five stages made here do not give reconstruct_views' result")
    torch.cuda.synchronize()
    ms = {name: [] for name in list(calls) + list(host)}
    stages = {}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.iters)
        for name, fn in host.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
        # the stages of one reconstruct_views call
        ev = [("start", torch.cuda.Event(enable_timing=True))]
        ev[0][1].record()

        def mark(stage):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((stage, e))

        reconstruct_stages(r["kp"], r["K"], r["seeds"], mark)
        torch.cuda.synchronize()
        for (_, a0), (stage, a1) in zip(ev, ev[1:]):
            stages.setdefault(stage, []).append(a0.elapsed_time(a1))
    lines = []
    for name in ms:
        res = {"call": name, "iters": args.iters if name in calls else 1, "rounds": args.rounds, "ms_per_call_median": round(float(np.median(ms[name])), 4),
               "ms_per_call_min": round(float(np.min(ms[name])), 4), "ms_per_call_max": round(float(np.max(ms[name])), 4),
               "device": torch.cuda.get_device_name(0)}
        if name in extra:
            res.update(extra[name](calls[name]()))
        if name == "reconstruct_views V=4":
            res["stage_ms_median"] = {k: round(float(np.median(v)), 4) for k, v in stages.items()}
        print(json.dumps(res), flush=True)
        lines.append(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
