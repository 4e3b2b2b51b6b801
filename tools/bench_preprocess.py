"""Benchmark of the on-device image preprocessing (roma_amd.preprocess_images, csrc/preprocess.hip) against the host path it
replaces, on the workload that feeds one flagship step: 16 decoded photographs (uint8, 1200 x 1600) resized to 560 x 560 and
864 x 864 and normalised.
  A  host    the loop of matcher._pil_to_normalised (PIL bicubic resize, / 255, mean / std, one image and one size at a time)
             followed by .to(device): 32 resizes and 32 float32 uploads - the code match() runs today;
  B  device  one preprocess_images call from the same host arrays, the single uint8 upload included.
Both legs run interleaved (A B A B) in one process after a warm-up; each leg is a host clock around work that ends in a device
synchronise; median and min - max over --rounds rounds.  The device time of the three kernels alone comes from the library's
per-launch events (roma_profile_enable) in a pass of its own.  The two legs' outputs are compared bit for bit.  One JSON line,
appended to --out (profiles/preprocess_bench.jsonl) and printed.
Usage: python tools/bench_preprocess.py [--rounds 7] [--images 16] [--height 1200] [--width 1600]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def photographs(n, h, w, seed=0):
    """n smooth uint8 images with texture: low-frequency colour fields plus noise (the resize cost does not depend on the content)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for i in range(n):
        f = rng.uniform(0.002, 0.02, size=(3, 2)).astype(np.float32)
        base = np.stack([127 + 90 * np.sin(f[c, 0] * xx + i) * np.cos(f[c, 1] * yy - i) for c in range(3)], axis=-1)
        out.append(np.clip(base + rng.normal(0, 12, size=(h, w, 3)), 0, 255).astype(np.uint8))
    return out


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--sizes", type=int, nargs=2, default=[560, 864])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_preprocess.py measures the device path: it needs a GPU"
    assert args.rounds >= 7, "at least 7 rounds"
    from PIL import Image
    import roma_amd
    from roma_amd import _lib
    from roma_amd.matcher import _pil_to_normalised
    sizes = [(s, s) for s in args.sizes]
    arrays = photographs(args.images, args.height, args.width)
    pils = [Image.fromarray(a) for a in arrays]  # decoded images, as match() holds them after Image.open

    def host():
        return [torch.stack([_pil_to_normalised(im, hw).to(DEV) for im in pils]) for hw in sizes]

    def device():
        return roma_amd.preprocess_images(arrays, sizes, device=DEV)

    for fn in (host, device, device):  # warm-up: code objects, the pinned and device allocations
        fn()
    torch.cuda.synchronize()
    ms = {"host ms": [], "device ms": []}
    for _ in range(args.rounds):
        for key, fn in (("host ms", host), ("device ms", device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    a, b = host(), device()
    equal = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))

    lib = _lib.load()
    lib.roma_profile_enable(1)
    for _ in range(args.rounds):
        device()
    torch.cuda.synchronize()
    n = lib.roma_profile_report(None, 0)
    buf = C.create_string_buffer(int(n))
    lib.roma_profile_report(buf, n)
    lib.roma_profile_enable(0)
    prof = json.loads(buf.value.decode())
    kernels = {k: round(v["total_ms"] / v["calls"], 4) for k, v in prof.items() if k.startswith("preprocess_")}

    px = sum(h * w for h, w in sizes)
    res = {"config": "preprocess", "images": args.images, "source": [args.height, args.width], "targets": sizes, "rounds": args.rounds,
           "uint8 upload MB": round(args.images * args.height * args.width * 3 / 1e6, 1),
           "float32 upload MB (host path)": round(args.images * px * 12 / 1e6, 1),
           **{k: stats(v) for k, v in ms.items()},
           "host over device": round(float(np.median(ms["host ms"]) / np.median(ms["device ms"])), 2),
           "device faster than host in every round": bool(np.max(ms["device ms"]) < np.min(ms["host ms"])),
           "kernel ms per call (library events, profiling pass)": kernels, "kernels ms": round(sum(kernels.values()), 4),
           "outputs bit-identical": bool(equal)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
