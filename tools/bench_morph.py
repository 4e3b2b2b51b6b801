"""Benchmark of the on-device warp morph rendering (roma_amd.render_morph, csrc/morph.hip) against the per-frame torch route of the
reference's demo/demo_3D_effect.py kept on the device, on the demo's own shape - B = 1, warp 864 x 1152, image 864 x 1152, T = 200
frames, uint8 out (597 MB of frames) - and on B = 8, 560 x 560, T = 24:
  A  torch   per frame: (1 - t) * warp[..., :2] + t * warp[..., 2:], F.grid_sample, clamp(0, 1) * 255, and one converting copy
             into the uint8 [H, W, 3] frame of a preallocated output - no host copy and no Pillow, which flatters it against the demo;
  B  hip     one roma_amd.render_morph call (two launches, nothing read back).
Both legs run interleaved (A B A B) in one process after a warm-up; each leg is a host clock around work that ends in a device
synchronise; median and min - max over --rounds rounds.  Reported with the ratio: leg B's frame bytes per second against the
6.29 TB/s that a float4 copy reaches on this device - the ceiling of a kernel that only stored its frames.  The two legs' frames
are compared under the uint8 rule of tests/morph_cases.py (at most one level apart, equal wherever 255 v of leg A's float frame is
not within 1e-3 of an integer).  One JSON line per shape, appended to --out (profiles/morph_bench.jsonl) and printed.  Reported,
not gated.
Usage: python tools/bench_morph.py [--rounds 7] [--shapes demo batch]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
COPY_CEILING_TBS = 6.29
SHAPES = {"demo": dict(B=1, H=864, W=1152, h=864, w=1152, T=200), "batch": dict(B=8, H=560, W=560, h=560, w=560, T=24)}


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def synthetic_warp(B, H, W, seed=0):
    """a seeded smooth warp with no weights needed: columns 0:2 the pixel centres, columns 2:4 a parallax-like smooth displacement of
    them that leaves the image at the borders"""
    ys = torch.linspace(-1 + 1 / H, 1 - 1 / H, H, device=DEV, dtype=torch.float64)
    xs = torch.linspace(-1 + 1 / W, 1 - 1 / W, W, device=DEV, dtype=torch.float64)
    y, x = torch.meshgrid(ys, xs, indexing="ij")
    g = torch.Generator("cpu").manual_seed(seed)
    out = []
    for _ in range(B):
        p = torch.rand(6, generator=g, dtype=torch.float64).tolist()
        bx = 1.04 * x + 0.08 * torch.sin(2.0 * y + 6.0 * p[0]) * torch.cos(1.5 * x + 6.0 * p[1]) + 0.06 * (p[2] - 0.5)
        by = 1.03 * y + 0.06 * torch.cos(2.5 * x + 6.0 * p[3]) * torch.sin(1.2 * y + 6.0 * p[4]) + 0.06 * (p[5] - 0.5)
        out.append(torch.stack((x, y, bx, by), dim=-1))
    return torch.stack(out).float().contiguous()


def run(name, shape, rounds):
    import roma_amd
    B, H, W, h, w, T = (shape[k] for k in ("B", "H", "W", "h", "w", "T"))
    warp = synthetic_warp(B, H, W)
    gen = torch.Generator(DEV).manual_seed(1)
    # uniform random float32: a picture derived from uint8 puts 255 v exactly on integers wherever a frame shows a texel unblended
    image = torch.rand((B, 3, h, w), generator=gen, device=DEV, dtype=torch.float32)
    ts = roma_amd.morph_times(T)
    ts_dev = torch.from_numpy(ts).to(DEV)
    out_a = torch.empty((B, T, H, W, 3), device=DEV, dtype=torch.uint8)
    coords_a, coords_b = warp[..., :2], warp[..., 2:]

    def frame_float(t):
        return F.grid_sample(image, (1 - t) * coords_a + t * coords_b, mode="bilinear", align_corners=False)

    def leg_torch():
        for i, t in enumerate(ts.tolist()):
            out_a[:, i].copy_((frame_float(t).clamp(0.0, 1.0) * 255).permute(0, 2, 3, 1))
        return out_a

    def leg_hip():
        return roma_amd.render_morph(warp, image, ts_dev)

    for fn in (leg_torch, leg_hip, leg_torch, leg_hip):  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    ms = {"torch ms": [], "hip ms": []}
    for _ in range(rounds):
        for key, fn in (("torch ms", leg_torch), ("hip ms", leg_hip)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    # the two legs' frames under the uint8 rule, frame by frame on the device
    got = leg_hip()
    leg_torch()
    n_diff = n_unexcused = n_excused = worst = 0
    for i, t in enumerate(ts.tolist()):
        v = frame_float(t).permute(0, 2, 3, 1).double()
        exc = ((v * 255 - torch.round(v * 255)).abs() < 1e-3) & (v != 0) & (v != 1)
        d = (got[:, i].to(torch.int16) - out_a[:, i].to(torch.int16)).abs()
        n_diff += int((d != 0).sum())
        n_unexcused += int(((d != 0) & ~exc).sum())
        n_excused += int(exc.sum())
        worst = max(worst, int(d.max()))
    frame_bytes = B * T * H * W * 3
    hip_med = float(np.median(ms["hip ms"]))
    tbs = frame_bytes / (hip_med * 1e-3) / 1e12
    res = {"config": "morph", "shape": name, "batch": B, "warp": [H, W], "image": [h, w], "frames": T, "frame bytes": frame_bytes,
           "rounds": rounds, **{k: stats(v) for k, v in ms.items()},
           "torch over hip": round(float(np.median(ms["torch ms"])) / hip_med, 2),
           "hip faster than torch in every round": bool(np.max(ms["hip ms"]) < np.min(ms["torch ms"])),
           "hip frame TB/s": round(tbs, 3), "copy ceiling TB/s": COPY_CEILING_TBS, "share of the copy ceiling": round(tbs / COPY_CEILING_TBS, 3),
           "values that differ": n_diff, "largest difference": worst, "differences outside the excused values": n_unexcused,
           "excused share": round(n_excused / frame_bytes, 5),
           "uint8 rule holds": bool(worst <= 1 and n_unexcused == 0 and n_excused <= 0.005 * frame_bytes)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", nargs="+", default=["demo", "batch"], choices=sorted(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_morph.py measures the device path: it needs a GPU"
    assert args.rounds >= 7, "at least 7 rounds"
    for name in args.shapes:
        line = json.dumps(run(name, SHAPES[name], args.rounds))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
