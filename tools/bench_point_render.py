"""Microbenchmark of point-cloud rendering (roma_amd.render_points; csrc/point_render.hip), after the method of
tools/bench_depth_fusion.py: the calls are timed alternately in --rounds rounds of --iters calls each, device events around each
block after a warm-up of every call, medians over the rounds.

  cloud              two views' worth of a dense reconstruction at 864 x 864 (1 492 992 rows in (view, pixel) order, made on the
                     device): a tilted plane behind a smaller nearer one, each view's pixels unprojected to the surface it sees
  render_points      into 60 frames of 864 x 1152 (a turntable, `orbit_cameras`) and into 1 frame; each with the defaults (radius 1,
                     occlusion filter, fill) and as the plain z-buffer (radius 0, both passes off), with colours
  torch yardstick    the same device, less work: projection, int64 keys, `scatter_reduce_(amin)` and a gather at radius 0, frame by
                     frame - no splat window, no filter, no fill, no colour.  It is checked to give the operator's depth and index
  kernels            the time of the clear and of each of the three kernels, from the library's per-launch events in a pass of their
                     own; for the splat kernel its offers - the (row, pixel) pairs it offers a key to, counted from `stats`: rows
                     whose cell lies inside the frame times the window, so splats clipped at the border count in full and rows
                     that only reach in from outside do not - over its time
  early-out A/B      --ab-lib PATH: a bench-only build of the library (`make -C roma_amd/csrc render_ab`) whose splat kernel
                     sends every offer as a 64-bit atomicMin, without the plain load in front of it.  Both libraries render the
                     same frames through the C entry, alternately, in this process; the outputs are checked to be identical.  In
                     that build every offer is an atomic: its offers per second are the 8-byte atomic minima per second

One JSON line per call appended to profiles/point_render_bench.jsonl.
Usage: python tools/bench_point_render.py [--iters 20] [--rounds 9] [--ab-lib roma_amd/libroma_hip_render_ab.so] [--out ...]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G = 864           # the grid of a view of the reconstruction
H, W = 864, 1152  # the frames
CENTRE = (0.0, 0.0, 5.5)


def cloud(dev):
    """(points [N, 3] f32, colors [N, 3] u8): the pixels of two views at G x G unprojected onto what they see - the plane z = 6 + 0.3 x
    - 0.2 y, or the nearer rectangle |x| < 0.9, |y| < 0.6 at z = 4 where the ray meets it"""
    f = 1.1 * G
    pts = []
    for v in range(2):
        c0 = torch.tensor([0.4 * v - 0.2, 0.0, 0.0], device=dev, dtype=torch.float64)
        c, r = torch.meshgrid(torch.arange(G, device=dev, dtype=torch.float64) + 0.5, torch.arange(G, device=dev, dtype=torch.float64) + 0.5, indexing="xy")
        d = torch.stack([(c - G / 2.0) / f, (r - G / 2.0) / f, torch.ones_like(c)], dim=-1).reshape(-1, 3)
        s_bg = (6.0 - c0[2] + 0.3 * c0[0] - 0.2 * c0[1]) / (d[:, 2] - 0.3 * d[:, 0] + 0.2 * d[:, 1])
        s_fg = (4.0 - c0[2]) / d[:, 2]
        hit = c0 + s_fg[:, None] * d
        s = torch.where((hit[:, 0].abs() < 0.9) & (hit[:, 1].abs() < 0.6), s_fg, s_bg)
        pts.append((c0 + s[:, None] * d).to(torch.float32))
    pts = torch.cat(pts)
    g = torch.Generator(device=dev).manual_seed(7)
    return pts, torch.randint(0, 256, (len(pts), 3), device=dev, dtype=torch.uint8, generator=g)


def torch_route(points, K, R, t):
    """radius 0, frame by frame: projection in the operator's order of operations, int64 keys, scatter_reduce_(amin), gather"""
    X = points.double()
    n = torch.arange(len(points), device=points.device, dtype=torch.int64)
    depth, index = [], []
    for k in range(len(R)):
        y = [((R[k, i, 0] * X[:, 0] + R[k, i, 1] * X[:, 1]) + R[k, i, 2] * X[:, 2]) + t[k, i] for i in range(3)]
        zf = y[2].float()
        u, v = K[0, 0] * (y[0] / y[2]) + K[0, 2], K[1, 1] * (y[1] / y[2]) + K[1, 2]
        fu, fv = torch.floor(u), torch.floor(v)
        ok = torch.isfinite(points).all(dim=1) & (y[2] >= 1e-6) & (zf > 0) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        key = (zf.view(torch.int32).to(torch.int64) << 32) | n
        cell = (fv.to(torch.int64) * W + fu.to(torch.int64))[ok]
        buf = torch.full((H * W,), torch.iinfo(torch.int64).max, device=points.device, dtype=torch.int64)
        buf.scatter_reduce_(0, cell, key[ok], "amin", include_self=True)
        have = buf != torch.iinfo(torch.int64).max
        row = torch.where(have, buf & 0xFFFFFFFF, -1)
        depth.append(torch.where(have, zf[row.clamp(min=0)], float("nan")).reshape(H, W))
        index.append(row.to(torch.int32).reshape(H, W))
    return torch.stack(depth), torch.stack(index)


def bind(path):
    """another build of the library, bound like roma_amd._lib binds its own"""
    from roma_amd import _lib
    lib = C.CDLL(path)
    for name in ("roma_op_render_points", "roma_op_render_points_workspace", "roma_profile_enable", "roma_profile_report", "roma_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def raw_call(lib, points, colors, K, R, t, kw):
    """the C entry on buffers made once; returns (run, outputs)"""
    dev, Cn, N = points.device, len(R), len(points)
    Kc = K[None].expand(Cn, 3, 3).contiguous()
    nws = int(lib.roma_op_render_points_workspace(1, Cn, H, W))
    ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
    out = (torch.empty((Cn, H, W, 3), device=dev, dtype=torch.uint8), torch.empty((Cn, H, W), device=dev, dtype=torch.float32),
           torch.empty((Cn, H, W), device=dev, dtype=torch.int32), torch.empty((Cn, H, W), device=dev, dtype=torch.uint8),
           torch.zeros((Cn, 4), device=dev, dtype=torch.int32))
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def run():
        rc = lib.roma_op_render_points(p(points), p(colors), None, None, p(Kc), p(R), p(t), 1, N, Cn, H, W, kw["radius"], 1e-6, math.inf,
                                       kw["occlusion_radius"], 0.05, 3, kw["fill_radius"], 3, 0, p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                       p(out[4]), p(ws), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise SystemExit("bench_point_render: " + lib.roma_last_error().decode())
    return run, out


def stage_ms(lib, fn, iters):
    lib.roma_profile_enable(1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    n = lib.roma_profile_report(None, 0)
    buf = C.create_string_buffer(int(n))
    lib.roma_profile_report(buf, n)
    lib.roma_profile_enable(0)
    return {k: round(v["total_ms"] / v["calls"], 4) for k, v in json.loads(buf.value.decode()).items() if k.startswith("render_")}


def timed(calls, rounds, iters):
    """alternating rounds; ms per call of every entry of calls: name -> (fn, iterations of a round)"""
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, (fn, it) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(it):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / it)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--ab-lib", default=None, help="a build with -DROMA_RENDER_NO_EARLY_OUT (make -C roma_amd/csrc render_ab)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_render_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_render: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import _lib, orbit_cameras, render_points
    dev = "cuda:0"
    lib = _lib.load()
    ab = bind(args.ab_lib) if args.ab_lib else None
    points, colors = cloud(dev)
    N = len(points)
    K = torch.tensor([[1000.0, 0.0, W / 2.0 + 0.13], [0.0, 1000.0, H / 2.0 - 0.21], [0.0, 0.0, 1.0]], device=dev, dtype=torch.float64)
    configs = {"defaults": dict(radius=1, occlusion_radius=2, fill_radius=1), "z-buffer": dict(radius=0, occlusion_radius=0, fill_radius=0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for Cn in (args.frames, 1):
        angles = np.linspace(-0.5, 0.5, Cn) if Cn > 1 else [0.2]
        R, t = orbit_cameras(np.eye(3), np.zeros(3), CENTRE, angles, device=dev)
        for cname, kw in configs.items():
            render = lambda: render_points(points, K, R, t, H, W, colors=colors, **kw)  # noqa: E731
            calls = {f"render_points {cname} C={Cn}": (render, args.iters)}
            if cname == "z-buffer":
                calls[f"torch scatter_reduce amin C={Cn}"] = (lambda: torch_route(points, K, R, t), 1)
            raws = {}
            if ab is not None:
                raws = {"early-out": raw_call(lib, points, colors, K, R, t, kw), "every offer an atomic": raw_call(ab, points, colors, K, R, t, kw)}
                for name, (run, _) in raws.items():
                    calls[f"C entry, {name}, {cname} C={Cn}"] = (run, args.iters)
            for fn, _ in calls.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            out = render()
            if cname == "z-buffer":
                d, i = torch_route(points, K, R, t)
                if not (torch.equal(torch.nan_to_num(out.depth, nan=-1.0), torch.nan_to_num(d, nan=-1.0)) and torch.equal(out.index, i)):
                    raise SystemExit("bench_point_render: the torch yardstick does not give the operator's depth and index")
                del d, i
            for name, (_, o) in raws.items():
                for a, b in zip(out, o):
                    if not torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)):
                        raise SystemExit(f"bench_point_render: the C entry ({name}) does not give render_points' outputs")
            ms = timed(calls, args.rounds, args.iters)
            stages = {"early-out": stage_ms(lib, render, args.iters)}
            if ab is not None:
                stages["every offer an atomic"] = stage_ms(ab, raws["every offer an atomic"][0], args.iters)
            stats = out.stats.cpu().numpy().astype(np.int64)
            offers = int(stats[:, 0].sum()) * (2 * kw["radius"] + 1) ** 2
            for name in ms:
                res = {"call": name, "iters": calls[name][1], "rounds": args.rounds, "ms_per_call_median": round(float(np.median(ms[name])), 4),
                       "ms_per_call_min": round(float(np.min(ms[name])), 4), "ms_per_call_max": round(float(np.max(ms[name])), 4),
                       "device": torch.cuda.get_device_name(0), "N": N, "C": Cn, "frame": [H, W]}
                if name.startswith("render_points"):
                    res.update({"config": kw, "stats_sum": stats.sum(axis=0).tolist(), "splat_offers": offers, "stage_ms": stages["early-out"],
                                "ms_per_frame": round(float(np.median(ms[name])) / Cn, 4)})
                    sp = stages["early-out"].get("render_splat_kernel")
                    if sp:
                        res["splat_offers_per_s"] = round(offers / (sp * 1e-3), 1)
                    yard = f"torch scatter_reduce amin C={Cn}"
                    if yard in ms:
                        res["torch_yardstick_over_this"] = round(float(np.median(ms[yard]) / np.median(ms[name])), 2)
                if name.startswith("C entry, every"):
                    sp = stages["every offer an atomic"].get("render_splat_kernel")
                    res.update({"stage_ms": stages["every offer an atomic"], "splat_offers": offers,
                                "splat_atomics_per_s": round(offers / (sp * 1e-3), 1) if sp else None,
                                "splat_ms_over_early_out": round(sp / stages["early-out"]["render_splat_kernel"], 3) if sp else None})
                print(json.dumps(res), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(res) + "\n")
            del out, raws, calls
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
