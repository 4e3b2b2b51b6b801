"""Microbenchmark of TSDF integration and mesh extraction (roma_amd.integrate_depth_maps, roma_amd.extract_mesh; csrc/tsdf.hip),
after the method of tools/bench_point_render.py: the calls are timed alternately in --rounds rounds of --iters calls each, device
events around each block after a warm-up of every call, medians (min - max) over the rounds.

  scene              8 views of 864 x 864 of a tilted plane behind a smaller nearer rectangle, the depth maps made on the device
  volumes            256^3 and 512 x 512 x 256 (nz = 256) around the scene, cubic voxels, trunc = 4 voxels, no colour
  integrate          the 8 views in one call into a volume that is NOT reset between calls: every call does the same work (the
                     weights saturate at max_weight, the means stay put), and a reset would add a memset to the time
  extract_mesh       from the integrated volume, with the default max_vertices / max_faces
  torch yardstick    the same device, the same update view by view in tensor arithmetic - the voxel centres in float64, project,
                     gather, where - on a fresh volume.  It is checked to give the operator's tsdf and weight in every bit before it
                     is timed
  kernels            the time of each kernel from the library's per-launch events, in a pass of their own; for the integration
                     kernel the bytes it must move when every voxel is touched (tsdf and weight read and written, 16 B a voxel)
                     over its time, against the 6.3 TB/s that a streaming kernel achieves on this device

One JSON line per call appended to profiles/tsdf_bench.jsonl.
Usage: python tools/bench_tsdf.py [--iters 10] [--rounds 7] [--out ...]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, V = 864, 8
HBM_ACHIEVABLE = 6.3e12  # bytes / s
VOLUMES = {"256^3": (256, 256, 256), "512x512x256": (256, 512, 512)}


def scene(dev):
    """(depth [V, G, G] f32, K [3, 3], R [V, 3, 3], t [V, 3]) f64: cameras on a ring in the plane z = 0, all looking along z; the
    plane z = 6 + 0.3 x - 0.2 y, or the nearer rectangle |x| < 0.9, |y| < 0.6 at z = 4 where the ray meets it"""
    f = 1.1 * G
    K = torch.tensor([[f, 0.0, G / 2.0 + 0.13], [0.0, f, G / 2.0 - 0.21], [0.0, 0.0, 1.0]], device=dev, dtype=torch.float64)
    c, r = torch.meshgrid(torch.arange(G, device=dev, dtype=torch.float64) + 0.5, torch.arange(G, device=dev, dtype=torch.float64) + 0.5, indexing="xy")
    d = torch.stack([(c - K[0, 2]) / f, (r - K[1, 2]) / f, torch.ones_like(c)], dim=-1)
    depth, t = [], []
    for v in range(V):
        phi = 2.0 * np.pi * v / V
        c0 = torch.tensor([0.6 * np.cos(phi), 0.4 * np.sin(phi), 0.0], device=dev, dtype=torch.float64)
        s_bg = (6.0 + 0.3 * c0[0] - 0.2 * c0[1]) / (d[..., 2] - 0.3 * d[..., 0] + 0.2 * d[..., 1])
        hit = c0 + 4.0 * d
        depth.append(torch.where((hit[..., 0].abs() < 0.9) & (hit[..., 1].abs() < 0.6), torch.full_like(s_bg, 4.0), s_bg).to(torch.float32))
        t.append(-c0)
    return torch.stack(depth), K, torch.eye(3, device=dev, dtype=torch.float64).expand(V, 3, 3).contiguous(), torch.stack(t)


def torch_route(vol, depth, K, R, t, max_weight, near):
    """the operator's update in the operator's order of operations, view by view, on the tensors of vol (in place)"""
    nz, ny, nx = vol.tsdf.shape
    dev = vol.tsdf.device
    vs, trunc = vol.voxel_size, vol.trunc
    ax = [vol.origin[a] + (torch.arange(n, device=dev, dtype=torch.float64) + 0.5) * vs for a, n in enumerate((nx, ny, nz))]
    X0, X1, X2 = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
    H, W = depth.shape[-2:]
    T, Wt = vol.tsdf, vol.weight
    for v in range(len(depth)):
        y0 = ((R[v, 0, 0] * X0 + R[v, 0, 1] * X1) + R[v, 0, 2] * X2) + t[v, 0]
        y1 = ((R[v, 1, 0] * X0 + R[v, 1, 1] * X1) + R[v, 1, 2] * X2) + t[v, 1]
        z = ((R[v, 2, 0] * X0 + R[v, 2, 1] * X1) + R[v, 2, 2] * X2) + t[v, 2]
        fu, fv = torch.floor(K[0, 0] * (y0 / z) + K[0, 2]), torch.floor(K[1, 1] * (y1 / z) + K[1, 2])
        live = (z > near) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        cell = torch.where(live, fv * W + fu, torch.zeros_like(fu)).to(torch.int64)
        d = depth[v].reshape(-1)[cell]
        sdf = d.double() - z
        live &= torch.isfinite(d) & (d > 0) & ~(sdf < -trunc)
        q = sdf / trunc
        f = torch.where(q < 1.0, q, torch.ones_like(q)).float()
        den = Wt + 1.0
        T.copy_(torch.where(live, (Wt * T + f) / den, T))  # w = 1: w * f is f
        Wt.copy_(torch.where(live, torch.clamp(den, max=max_weight), Wt))
    return vol


def stage_ms(lib, fn, iters, prefixes):
    lib.roma_profile_enable(1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    n = lib.roma_profile_report(None, 0)
    buf = C.create_string_buffer(int(n))
    lib.roma_profile_report(buf, n)
    lib.roma_profile_enable(0)
    return {k: round(v["total_ms"] / v["calls"], 4) for k, v in json.loads(buf.value.decode()).items() if k.startswith(prefixes)}


def timed(calls, rounds):
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import _lib, extract_mesh, integrate_depth_maps, tsdf_volume
    dev = "cuda:0"
    lib = _lib.load()
    depth, K, R, t = scene(dev)
    kw = dict(max_weight=64.0, near=1e-6)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for vname, dims in VOLUMES.items():
        nz, ny, nx = dims
        vs = 6.0 / nx
        origin = torch.tensor([-0.5 * nx * vs, -0.5 * ny * vs, 5.5 - 0.5 * nz * vs], device=dev, dtype=torch.float64)
        vs_t = torch.tensor(vs, device=dev, dtype=torch.float64)
        fresh = lambda: tsdf_volume(dims, origin, vs_t, 4.0 * vs_t)  # noqa: E731
        vol = integrate_depth_maps(fresh(), depth, K, R, t, **kw)
        yard = torch_route(fresh(), depth, K, R, t, kw["max_weight"], kw["near"])
        if not (torch.equal(vol.tsdf, yard.tsdf) and torch.equal(vol.weight, yard.weight)):
            raise SystemExit("bench_tsdf: the torch yardstick does not give the operator's tsdf and weight")
        touched = int((vol.weight > 0).sum())
        del yard
        scratch = fresh()
        calls = {f"integrate_depth_maps V={V} {vname}": (lambda: integrate_depth_maps(vol, depth, K, R, t, **kw), args.iters),
                 f"extract_mesh {vname}": (lambda: extract_mesh(vol, min_weight=1.0), args.iters),
                 f"torch view by view V={V} {vname}": (lambda: torch_route(scratch, depth, K, R, t, kw["max_weight"], kw["near"]), 1)}
        for fn, _ in calls.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        mesh = extract_mesh(vol, min_weight=1.0)
        ms = timed(calls, args.rounds)
        stages = stage_ms(lib, calls[f"integrate_depth_maps V={V} {vname}"][0], args.iters, "tsdf_")
        stages.update(stage_ms(lib, calls[f"extract_mesh {vname}"][0], args.iters, "mesh_"))
        nominal = 16.0 * nz * ny * nx
        for name in ms:
            res = {"call": name, "iters": calls[name][1], "rounds": args.rounds, "ms_per_call_median": round(float(np.median(ms[name])), 4),
                   "ms_per_call_min": round(float(np.min(ms[name])), 4), "ms_per_call_max": round(float(np.max(ms[name])), 4),
                   "device": torch.cuda.get_device_name(0), "views": [V, G, G], "dims": list(dims), "voxels_touched": touched}
            if name.startswith("integrate"):
                k_ms = stages["tsdf_integrate_kernel"]
                res.update({"stage_ms": {k: v for k, v in stages.items() if k.startswith("tsdf_")}, "bytes_when_every_voxel_is_touched": nominal,
                            "kernel_bytes_per_s": round(nominal / (k_ms * 1e-3), 1), "fraction_of_6.3_TB_per_s": round(nominal / (k_ms * 1e-3) / HBM_ACHIEVABLE, 4),
                            "torch_yardstick_over_this": round(float(np.median(ms[f"torch view by view V={V} {vname}"]) / np.median(ms[name])), 2)})
            if name.startswith("extract"):
                res.update({"stage_ms": {k: v for k, v in stages.items() if k.startswith("mesh_")}, "counts": mesh.counts.cpu().tolist(),
                            "totals": mesh.totals.cpu().tolist(), "stats": mesh.stats.cpu().tolist()})
            print(json.dumps(res), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        del vol, scratch, mesh, calls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
