"""Microbenchmark of the device RANSAC (roma_amd.geometry, csrc/geometry.hip) at the settings of the reference's consumers:

  * find_fundamental at B = 8, N = 10 000, threshold 0.2 px, confidence 0.999999, max_iters 10 000 (demo_fundamental), on the
    relief scene of accuracy_harness.synthetic_relief_pair with 0 % and 30 % uniform outliers;
  * find_homography at B = 8, N = 5 000 with the HPatches benchmark's settings (threshold 3 min(w, h) / 480 at 864^2,
    confidence 0.99999, OpenCV's default 2 000 iterations), 0.5 px noise and 30 % outliers.

Each configuration runs twice at the same settings: plain RANSAC + LO (`ransac`, the default of find_*) and MAGSAC++ scoring
with IRLS local optimisation (`magsac`, method="magsac").  Per leg one JSON line: ms per batched call (device events, after
warm-up), model-point evaluations per second (the hypotheses the score kernel ran x models per hypothesis x points), rounds
executed per pair, and the same work through tools/geometry_ref.py / tools/magsac_ref.py on the host (numpy f64, one pair after
the other) - a CPU number, for scale only.
--lm measures the Levenberg-Marquardt refinement (csrc/model_refine.hip) instead: the HPatches homography call (B = 8,
N = 5 000, 0.5 px noise) and demo_fundamental's call (B = 8, N = 10 000, 0.1 px noise) at 0 % and 30 % outliers, the default
call against the same call with lm_steps=10 in one process, timed alternately in rounds, medians over the rounds; one JSON
line per configuration with the added time, refine_* alone and the fit's counters.  --parent-lib DIR (a directory holding another
build of libroma_hip.so, e.g. the parent commit's) adds that build's two calls to the same alternation, and compares the
outputs build against build, bit for bit: the default call, refine_* on the bench batch and refine_* on a ragged batch
(`ragged_batch`).  Without --lm, --parent-lib adds one line per configuration (`against_parent`): every output of `ransac` and
`magsac` on the bench batch and on the ragged batch of the pipeline (`pipeline_counts`) build against build, and both builds
timed alternately over --rounds.
Usage: python tools/bench_geometry.py [--iters 20] [--no-cpu] [--method ransac|magsac|both] [--rounds 7] [--parent-lib DIR]
       python tools/bench_geometry.py --lm [--iters 20] [--rounds 7] [--parent-lib DIR]
"""
import argparse
import contextlib
import ctypes
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import geometry_ref as gr  # noqa: E402
import magsac_ref as mr  # noqa: E402
from accuracy_harness import synthetic_relief_pair  # noqa: E402


def relief_batch(B, N, outlier_frac, seed=0, h=480, w=640, noise=0.0):
    a, b = np.zeros((B, N, 2)), np.zeros((B, N, 2))
    for i in range(B):
        d = synthetic_relief_pair(h, w, seed=seed + i)
        m = d["gt_matches"].double().numpy().reshape(-1, 4)
        vis = np.nonzero(d["gt_certainty"].numpy().reshape(-1) > 0)[0]
        rng = np.random.default_rng(seed + i)
        sel = rng.choice(vis, N, replace=False)
        a[i] = np.stack([(m[sel, 0] + 1) * w / 2, (m[sel, 1] + 1) * h / 2], 1)
        b[i] = np.stack([(m[sel, 2] + 1) * w / 2, (m[sel, 3] + 1) * h / 2], 1)
        out = rng.random(N) < outlier_frac
        b[i, out] = rng.uniform([0, 0], [w, h], (out.sum(), 2))
        if noise:  # drawn last: the noise-free batches are what they were
            b[i] += noise * rng.normal(size=(N, 2))
    return a, b


def homography_batch(B, N, outlier_frac, seed=0, size=864):
    a, b = np.zeros((B, N, 2)), np.zeros((B, N, 2))
    for i in range(B):
        rng = np.random.default_rng(100 + seed + i)
        H = np.eye(3) + np.array([[0.1, 0.05, 20], [-0.05, 0.1, 15], [1e-4, 1e-4, 0]]) * rng.uniform(-1, 1, (3, 3))
        a[i] = rng.uniform(0, size, (N, 2))
        q = np.c_[a[i], np.ones(N)] @ H.T
        b[i] = q[:, :2] / q[:, 2:] + 0.5 * rng.normal(size=(N, 2))
        out = rng.random(N) < outlier_frac
        b[i, out] = rng.uniform(0, size, (out.sum(), 2))
    return a, b


def run(name, model, a, b, thr, conf, max_iters, iters, cpu, method="ransac"):
    from roma_amd.geometry import magsac, ransac
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    fn = ransac if method == "ransac" else magsac

    def call():
        return fn(model, da, db, thr, conf, max_iters, seed=seeds)[:4]
    for _ in range(3):
        M, mask, ok, info = call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        M, mask, ok, info = call()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    info = info.cpu().numpy()
    roots = gr.MAX_ROOTS if model == gr.FUNDAMENTAL else 1
    evals = float(info[:, 0].sum()) * gr.ROUND * roots * a.shape[1]
    res = {"config": name, "method": method, "B": int(a.shape[0]), "N": int(a.shape[1]), "threshold": thr, "confidence": conf, "max_iters": max_iters,
           "ms_per_call": round(ms, 4), "model_point_evals_per_s": evals / (ms * 1e-3), "rounds_per_pair": info[:, 0].tolist(),
           "inliers_per_pair": info[:, 4].tolist(), "ok": ok.cpu().tolist()}
    if cpu:
        t = time.perf_counter()
        rounds = []
        for i in range(len(a)):
            pa, pb = a[i].astype(np.float32).astype(np.float64), b[i].astype(np.float32).astype(np.float64)
            if method == "ransac":
                r = gr.ransac(model, pa, pb, thr, conf, max_iters, i + 1, True)
            else:
                r = mr.magsac(model, pa, pb, thr, conf, max_iters, i + 1)
            rounds.append(r["rounds"])
        res["cpu_numpy_reference_ms_per_call"] = round((time.perf_counter() - t) * 1e3, 1)
        res["cpu_reference_rounds_per_pair"] = rounds
    print(json.dumps(res), flush=True)
    return res


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def _other_build(directory):
    """another build of libroma_hip.so, bound with the signatures it has"""
    from roma_amd import _lib
    lib = ctypes.CDLL(os.path.join(directory, "libroma_hip.so"))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    lib.h16 = "bf16"
    return lib


@contextlib.contextmanager
def _using(lib):
    """roma_amd's calls go to `lib` inside the block (None: the in-tree build)"""
    from roma_amd import _lib
    mine = _lib.load()
    if lib is not None:
        _lib._libs["bf16"] = lib
    try:
        yield
    finally:
        _lib._libs["bf16"] = mine


def same_bits(x, y):
    """torch.equal of the bit patterns: a NaN equals itself"""
    if x.is_floating_point():
        x, y = x.view(torch.int64 if x.dtype == torch.float64 else torch.int32), y.view(torch.int64 if y.dtype == torch.float64 else torch.int32)
    return bool(torch.equal(x, y))


def outputs_equal(parent, call, names):
    """{name: this build's output equals the parent build's}"""
    mine = call()
    with _using(parent):
        theirs = call()
    return {k: same_bits(x, y) for k, x, y in zip(names, mine, theirs)}


def within_spread(this, parent):
    """this build's median is at most the parent's plus the parent's own spread over its rounds"""
    return bool(np.median(this) <= np.median(parent) + (np.max(parent) - np.min(parent)))


def ragged_batch(a, b, min_rows, n=1000, counts=None):
    """the first n rows of pair 0 eight times, cut to the counts at which a workgroup's reduction can go wrong: threads and
    whole waves without rows, one row past a wave or the workgroup, exactly min_rows, one below it: (a, b, counts)"""
    counts = counts or (n, 513, 512, 511, 65, 64, min_rows, min_rows - 1)
    ra, rb = np.full((8, n, 2), np.nan), np.full((8, n, 2), np.nan)
    for i, c in enumerate(counts):
        ra[i, :c], rb[i, :c] = a[0, :c], b[0, :c]
    dev = lambda x: torch.tensor(x, dtype=torch.float32, device="cuda:0")  # noqa: E731
    return dev(ra), dev(rb), torch.tensor(counts, dtype=torch.int32, device="cuda:0")


def pipeline_counts(s):
    """rows per pair around the 64-row stride of the score and accept waves and the 256-row stride of the normalise, refit and
    mask workgroups of csrc/ransac.h, the sample size s and one below it"""
    return (513, 257, 256, 65, 64, 63, s, s - 1)


def against_parent(parent, calls, iters, rounds):
    """calls {name: fn -> tensors}.  Per call: whether every output of this build equals the parent build's bit for bit, and
    (rounds > 0) both builds timed alternately, `iters` calls per round: {name: {...}}"""
    res = {}
    for name, fn in calls.items():
        r = {"outputs equal the parent's": all(outputs_equal(parent, fn, itertools.count()).values())}
        ms = {"parent": [], "this": []}
        for _ in range(rounds):
            for k, lib in (("parent", parent), ("this", None)):
                with _using(lib):
                    ms[k].append(_timed(fn, iters)[0])
        if rounds:
            r.update({"this ms": _stats(ms["this"]), "parent ms": _stats(ms["parent"]),
                      "within the parent's spread": within_spread(ms["this"], ms["parent"])})
        res[name] = r
    return res


def compare_plain(name, model, a, b, thr, conf, max_iters, iters, rounds, parent):
    from roma_amd.geometry import magsac, ransac
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    s = 4 if model == gr.HOMOGRAPHY else 7
    ra, rb, counts = ragged_batch(a, b, s, counts=pipeline_counts(s))
    calls = {}
    for fn in (ransac, magsac):
        calls[fn.__name__] = lambda fn=fn: fn(model, da, db, thr, conf, max_iters, seed=seeds)
        calls[fn.__name__ + " ragged"] = lambda fn=fn: fn(model, ra, rb, thr, conf, 600, seed=seeds, counts=counts)
        calls[fn.__name__ + " ragged confidence=1"] = lambda fn=fn: fn(model, ra, rb, thr, 1.0, 600, seed=seeds, counts=counts)
    res = {"config": name + " against the parent build", "rounds": rounds, "iters_per_round": iters,
           **against_parent(parent, calls, iters, rounds)}
    print(json.dumps(res), flush=True)
    return res


def _stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def run_lm(name, model, a, b, thr, conf, max_iters, iters, rounds, parent, lm_steps=10):
    """default call, the same call with lm_steps, and the parent build's two calls if given: timed alternately"""
    from roma_amd.geometry import find_fundamental, find_homography, refine_fundamental, refine_homography
    find, fit = (find_homography, refine_homography) if model == gr.HOMOGRAPHY else (find_fundamental, refine_fundamental)
    da = torch.tensor(a, dtype=torch.float32, device="cuda:0")
    db = torch.tensor(b, dtype=torch.float32, device="cuda:0")
    seeds = torch.arange(len(a), dtype=torch.int64) + 1
    plain = lambda: find(da, db, thr, conf, max_iters, seed=seeds)  # noqa: E731
    fitted = lambda: find(da, db, thr, conf, max_iters, seed=seeds, lm_steps=lm_steps)  # noqa: E731
    legs = {"this ms": (None, plain), f"this lm_steps={lm_steps} ms": (None, fitted)}
    if parent is not None:
        legs = {"parent ms": (parent, plain), f"parent lm_steps={lm_steps} ms": (parent, fitted), **legs}
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
    M, mask, ok = plain()
    ms_fit, (M1, _, info, cost) = _timed(lambda: fit(M, da, db, thr, max_steps=lm_steps, valid=ok), iters)
    if parent is not None:
        with _using(parent):
            same = all(torch.equal(x, y) for x, y in zip(plain(), (M, mask, ok)))
        names = ("M", "mask", "info", "cost")
        refined = outputs_equal(parent, lambda: fit(M, da, db, thr, max_steps=lm_steps, valid=ok), names)
        # every row of the ragged batch starts from pair 0's model at its full count
        ra, rb, counts = ragged_batch(a, b, 4 if model == gr.HOMOGRAPHY else 7)
        M0 = find(ra[0], rb[0], thr, conf, max_iters, seed=1)[0]
        ragged = outputs_equal(parent, lambda: fit(M0.expand(8, 3, 3).contiguous(), ra, rb, thr, max_steps=lm_steps, counts=counts),
                               names)
    info, cost = info.cpu().numpy(), cost.cpu().numpy()
    res = {"config": name, "B": int(a.shape[0]), "N": int(a.shape[1]), "threshold": thr, "lm_steps": lm_steps, "rounds": rounds,
           "iters_per_round": iters, **{k: _stats(v) for k, v in ms.items()},
           "added by lm ms": round(float(np.median(ms[f"this lm_steps={lm_steps} ms"]) - np.median(ms["this ms"])), 4),
           "refine alone ms": round(ms_fit, 4), "steps_per_pair": info[:, 0].tolist(), "cost_evals_per_pair": info[:, 1].tolist(),
           "active_rows_per_pair": info[:, 2].tolist(), "cost_start": cost[:, 0].round(3).tolist(), "cost_end": cost[:, 1].round(3).tolist()}
    if parent is not None:
        res["default outputs equal the parent's"] = bool(same)
        res["refined outputs equal the parent's"] = refined
        res["ragged refined outputs equal the parent's"] = ragged
        res["lm within the parent's spread"] = within_spread(ms[f"this lm_steps={lm_steps} ms"], ms[f"parent lm_steps={lm_steps} ms"])
    print(json.dumps(res), flush=True)
    return res


def main_lm(args):
    parent = _other_build(args.parent_lib) if args.parent_lib else None
    B = 8
    for frac in (0.0, 0.3):
        a, b = homography_batch(B, 5000, frac)
        run_lm(f"find_homography hpatches outliers={frac}", gr.HOMOGRAPHY, a, b, 3 * 864 / 480, 0.99999, 2000, args.iters, args.rounds,
               parent)
    for frac in (0.0, 0.3):
        a, b = relief_batch(B, 10000, frac, noise=0.1)
        run_lm(f"find_fundamental demo_fundamental outliers={frac}", gr.FUNDAMENTAL, a, b, 0.2, 0.999999, 10000, args.iters,
               args.rounds, parent)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host reference timing")
    ap.add_argument("--method", choices=("ransac", "magsac", "both"), default="both")
    ap.add_argument("--lm", action="store_true", help="measure find_*(..., lm_steps=10) against the default call")
    ap.add_argument("--rounds", type=int, default=7, help="--lm, --parent-lib: alternating rounds per leg")
    ap.add_argument("--parent-lib", default=None, help="directory of another build of libroma_hip.so to time next to this one and compare outputs with")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_geometry.py measures the device path: it needs a GPU"
    if args.lm:
        return main_lm(args)
    methods = ("ransac", "magsac") if args.method == "both" else (args.method,)
    parent = _other_build(args.parent_lib) if args.parent_lib else None
    B = 8
    configs = [(f"find_fundamental demo_fundamental outliers={frac}", gr.FUNDAMENTAL, *relief_batch(B, 10000, frac), 0.2, 0.999999,
                10000) for frac in (0.0, 0.3)]
    configs.append(("find_homography hpatches outliers=0.3", gr.HOMOGRAPHY, *homography_batch(B, 5000, 0.3), 3 * 864 / 480, 0.99999,
                    2000))
    for cfg in configs:
        for m in methods:
            run(*cfg, args.iters, not args.no_cpu, m)
        if parent is not None:
            compare_plain(*cfg, args.iters, args.rounds, parent)


if __name__ == "__main__":
    main()
