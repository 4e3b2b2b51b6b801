"""Robust two-view geometry on the device (`roma_op_ransac`): what the reference's demos do with `sample()` output through
OpenCV - cv2.findHomography(..., cv2.RANSAC) (benchmarks/hpatches_sequences_homog_benchmark.py) and
cv2.findFundamentalMat(..., cv2.FM_RANSAC) (demo/demo_fundamental.py) - batched over pairs, in HIP (csrc/geometry.hip).

Plain RANSAC with OpenCV's adaptive iteration count, followed (refine=True) by up to three least-squares refits on the inliers
(local optimisation).  OpenCV's USAC_MAGSAC scoring, which demo_fundamental uses, is not restated: plain RANSAC + LO stands in
for it, and there is no Levenberg-Marquardt polish.  The algorithm is restated in numpy float64 by tools/geometry_ref.py.

Both models map A to B in pixel coordinates: x_B ~ H x_A and x_B^T F x_A = 0, like OpenCV's (points1 = A, points2 = B).  H and F
are scaled so that [2, 2] = 1 (unit Frobenius norm where |[2, 2]| < 1e-12 of it); F has rank 2.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

HOMOGRAPHY, FUNDAMENTAL = 0, 1
SAMPLE_SIZE = {HOMOGRAPHY: 4, FUNDAMENTAL: 7}
ROUND = 256  # hypotheses per pair and round (csrc/geometry.h RANSAC_ROUND)


def _as_batch(k: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(k, torch.Tensor) or not k.is_cuda:
        raise _lib.RomaHipError(f"roma_amd.geometry: {name} must be a tensor on a HIP device; there is no CPU fallback")
    if k.dim() not in (2, 3) or k.shape[-1] != 2:
        raise ValueError(f"roma_amd.geometry: {name} must be [N, 2] or [B, N, 2], got {tuple(k.shape)}")
    if k.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"roma_amd.geometry: {name} must be float32 or float64, got {k.dtype}")
    return k.detach().to(torch.float32).contiguous()


def ransac(model: int, kpts_A: torch.Tensor, kpts_B: torch.Tensor, threshold: float, confidence: float, max_iters: int,
           seed=None, refine: bool = True, counts=None):
    """Batched robust estimation, no host synchronisation.  kpts [B, N, 2] device pixel coordinates; counts [B] rows per pair
    (rows at or beyond counts[b] are never read); seed an int (every pair), a [B] tensor (one per pair) or None (drawn from
    torch's CPU generator).  Returns (M [B, 3, 3] float64, mask [B, N] bool, ok [B] bool, info [B, 6] int32) with
    info = (rounds run, winning hypothesis, its root, its inlier count, final inlier count, pair valid)."""
    a, b = _as_batch(kpts_A, "kpts_A"), _as_batch(kpts_B, "kpts_B")
    a = a[None] if a.dim() == 2 else a
    b = b[None] if b.dim() == 2 else b
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"roma_amd.geometry: kpts_A {tuple(kpts_A.shape)} and kpts_B {tuple(kpts_B.shape)} differ in shape")
    if a.device != b.device:
        raise ValueError("roma_amd.geometry: kpts_A and kpts_B live on different devices")
    if model not in SAMPLE_SIZE:
        raise ValueError(f"roma_amd.geometry: unknown model {model}")
    if not (threshold > 0) or not (0 <= confidence <= 1) or int(max_iters) <= 0:
        raise ValueError("roma_amd.geometry: need threshold > 0, 0 <= confidence <= 1, max_iters > 0")
    B, N, dev = int(a.shape[0]), int(a.shape[1]), a.device
    M = torch.zeros((B, 3, 3), device=dev, dtype=torch.float64)
    mask = torch.zeros((B, N), device=dev, dtype=torch.bool)
    ok = torch.zeros((B,), device=dev, dtype=torch.bool)
    info = torch.zeros((B, 6), device=dev, dtype=torch.int32)
    if B == 0:
        return M, mask, ok, info
    if counts is not None:
        counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if counts.shape[0] != B:
            raise ValueError(f"roma_amd.geometry: counts has {counts.shape[0]} entries for {B} pairs")
    if seed is None:
        seeds = torch.randint(0, 2 ** 62, (B,), dtype=torch.int64)  # CPU generator: no device synchronisation
    elif isinstance(seed, torch.Tensor):
        seeds = seed.reshape(-1).to(torch.int64)
        if seeds.shape[0] != B:
            raise ValueError(f"roma_amd.geometry: {seeds.shape[0]} seeds for {B} pairs")
    else:
        seeds = torch.full((B,), int(seed), dtype=torch.int64)
    seeds = seeds.to(dev).contiguous()  # read as uint64 by the kernels
    if N < SAMPLE_SIZE[model]:  # no pair can hold a minimal sample: nothing to launch
        return M, mask, ok, info
    lib = _lib.load()
    nws = int(lib.roma_op_ransac_workspace(B, N))
    ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(lib.roma_op_ransac(int(model), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                      C.c_void_p(counts.data_ptr() if counts is not None else 0), C.c_void_p(seeds.data_ptr()), B, N,
                                      float(threshold), float(confidence), int(max_iters), 1 if refine else 0,
                                      C.c_void_p(M.data_ptr()), C.c_void_p(mask.data_ptr()), C.c_void_p(ok.data_ptr()),
                                      C.c_void_p(info.data_ptr()), C.c_void_p(ws.data_ptr()), nws,
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return M, mask, ok, info


def _front(model, kpts_A, kpts_B, threshold, confidence, max_iters, seed, refine, counts):
    single = isinstance(kpts_A, torch.Tensor) and kpts_A.dim() == 2
    M, mask, ok, _ = ransac(model, kpts_A, kpts_B, threshold, confidence, max_iters, seed, refine, counts)
    if not single:
        return M, mask, ok
    if not bool(ok[0]):  # the one synchronisation of the single-pair form (OpenCV returns None)
        return None, None
    return M[0], mask[0]


def find_homography(kpts_A, kpts_B, ransac_reproj_threshold=3.0, confidence=0.995, max_iters=2000, seed=None, refine=True,
                    counts=None):
    """cv2.findHomography(kpts_A, kpts_B, cv2.RANSAC, ransac_reproj_threshold, maxIters=max_iters, confidence=confidence) on the
    device: 4-point DLT hypotheses (OpenCV's checkSubset), inliers |H x_A - x_B| < threshold in image B.

    kpts_A, kpts_B: [N, 2] -> (H [3, 3] float64, mask [N] bool) or (None, None) when no model was found;
    [B, N, 2] -> (H [B, 3, 3], mask [B, N], ok [B]) with no host synchronisation.  See `ransac` for seed and counts."""
    return _front(HOMOGRAPHY, kpts_A, kpts_B, ransac_reproj_threshold, confidence, max_iters, seed, refine, counts)


def find_fundamental(kpts_A, kpts_B, ransac_reproj_threshold=3.0, confidence=0.99, max_iters=1000, seed=None, refine=True,
                     counts=None):
    """cv2.findFundamentalMat(kpts_A, kpts_B, cv2.FM_RANSAC, ransac_reproj_threshold, confidence, max_iters) on the device:
    7-point hypotheses (up to 3 models each), inliers whose distances to both epipolar lines are below the threshold.

    kpts_A, kpts_B: [N, 2] -> (F [3, 3] float64, mask [N] bool) or (None, None) when no model was found;
    [B, N, 2] -> (F [B, 3, 3], mask [B, N], ok [B]) with no host synchronisation.  See `ransac` for seed and counts."""
    return _front(FUNDAMENTAL, kpts_A, kpts_B, ransac_reproj_threshold, confidence, max_iters, seed, refine, counts)
