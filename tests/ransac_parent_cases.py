"""The cases of tests/test_gpu_ransac_parent.py and tools/record_ransac_parent.py: every instantiation of the shared RANSAC
pipeline (csrc/ransac.h) - H, F and E under count and MAGSAC++ scoring, absolute pose under count scoring - on small ragged
batches around the 64-row waves, the one-or-two-round boundary, invalid pairs and the NaN-row convention.  CASES maps a name
to a function that runs the case through the public Python API and returns its output tensors; the fixture
tests/golden/ransac_parent.npz holds what they returned at the commit before absolute pose moved into the shared pipeline."""
import functools

import numpy as np
import torch

from absolute_pose_cases import THR, scene
from test_cpu_geometry import _homography_scene, relief_scene
from test_gpu_absolute_pose import _ragged_batch

DEV = "cuda:0"
SAMPLE = {"H": 4, "F": 7, "E": 5}
N = 257
ITERS = (256, 300)  # one round and two


def _dev(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=DEV)


# ---- absolute pose
def _ap_ragged(max_iters):
    from roma_amd.absolute_pose import absolute_pose
    K, X, kp, counts = _ragged_batch(np.nan)
    return absolute_pose(_dev(X), _dev(kp), K, THR, 1.0, max_iters, seed=torch.arange(31, 37), counts=torch.tensor(counts))


def _ap_adaptive():
    """the four pairs of test_gpu_absolute_pose.test_determinism_and_independence_of_the_batch: the adaptive count ends the sampling"""
    from roma_amd.absolute_pose import absolute_pose
    scenes = [scene(n=700, outlier_frac=f, noise_px=0.3, rng_seed=s) for f, s in ((0.2, 1), (0.4, 2), (0.1, 3), (0.5, 4))]
    X, kp = _dev(np.stack([s[3] for s in scenes])), _dev(np.stack([s[4] for s in scenes]))
    return absolute_pose(X, kp, scenes[0][0], THR, 0.9999, 600, seed=torch.tensor([11, 12, 13, 14]))


# ---- H, F, E
@functools.lru_cache(maxsize=None)
def two_view_batch(model):
    """B = 6 pairs of N = 257 rows, NaN beyond counts = (0, S - 1, S, 63, 65, 257); row 100 of the last pair is NaN as well.
    The pairs of test_gpu_geometry._fold_scene: 30 % gross outliers on a homography, or the relief with 0.3 px of noise (pixels).
    (A, B float32 [6, 257, 2], counts, threshold in pixels, K)"""
    S = SAMPLE[model]
    counts = [0, S - 1, S, 63, 65, 257]
    A, Bp = np.full((6, N, 2), np.nan, dtype=np.float32), np.full((6, N, 2), np.nan, dtype=np.float32)
    K = None
    for b, n in enumerate(counts):
        if n == 0:
            continue
        if model == "H":
            _, pa, pb, _ = _homography_scene(n=n, outlier_frac=0.3, seed=20 + b)
        else:
            K, _, _, _, pa, pb, _ = relief_scene(n=n, noise_px=0.3, thr=1.0, rng_seed=20 + b)
        A[b, :n], Bp[b, :n] = pa, pb
    A[5, 100] = np.nan
    return A, Bp, counts, 3.0 if model == "H" else 1.0, K


def _two_view(model, scoring, max_iters, option, with_K=False):
    """option: `refine` under count scoring (H, F), `lo_iters` under MAGSAC++; E takes pixels and K, or normalised coordinates"""
    from roma_amd import geometry as g
    A, Bp, counts, thr, K = two_view_batch(model)
    seeds, dc = torch.arange(41, 47, dtype=torch.int64), torch.tensor(counts)
    if model != "E":
        fn, opt = (g.magsac, {"lo_iters": option}) if scoring == "magsac" else (g.ransac, {"refine": bool(option)})
        return fn("HF".index(model), _dev(A), _dev(Bp), thr, 1.0, max_iters, seed=seeds, counts=dc, **opt)
    if not with_K:
        Ki = np.linalg.inv(K[:2, :2])
        A, Bp = ((p.astype(np.float64) - K[None, None, :2, 2]) @ Ki.T for p in (A, Bp))
        thr, K = thr / K[0, 0], None
    if scoring == "magsac":
        return g.essential_magsac(_dev(A), _dev(Bp), K, 1.0, thr, max_iters, seed=seeds, lo_iters=option, counts=dc)
    return g.essential(_dev(A), _dev(Bp), K, 1.0, thr, max_iters, seed=seeds, counts=dc)


def _cases():
    c = {"ap_adaptive": _ap_adaptive}
    for it in ITERS:
        c[f"ap_ragged_{it}"] = functools.partial(_ap_ragged, it)
        for m in "HF":
            for opt in (0, 1):
                c[f"{m}_count_{it}_refine{opt}"] = functools.partial(_two_view, m, "count", it, opt)
            for lo in (0, 3):
                c[f"{m}_magsac_{it}_lo{lo}"] = functools.partial(_two_view, m, "magsac", it, lo)
        for k in (0, 1):
            c[f"E_count_{it}_K{k}"] = functools.partial(_two_view, "E", "count", it, None, bool(k))
            for lo in (0, 3):
                c[f"E_magsac_{it}_K{k}_lo{lo}"] = functools.partial(_two_view, "E", "magsac", it, lo, bool(k))
    return c


CASES = _cases()
