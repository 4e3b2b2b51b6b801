"""Robust two-view geometry on the device (`roma_op_ransac`): what the reference's demos do with `sample()` output through
OpenCV - cv2.findHomography(..., cv2.RANSAC) (benchmarks/hpatches_sequences_homog_benchmark.py) and
cv2.findFundamentalMat(..., cv2.FM_RANSAC) (demo/demo_fundamental.py) - batched over pairs, in HIP (csrc/geometry.hip).

Plain RANSAC with OpenCV's adaptive iteration count, followed (refine=True) by up to three least-squares refits on the inliers
(local optimisation).  The algorithm is restated in numpy float64 by tools/geometry_ref.py.  lm_steps > 0 (default 0) adds what
OpenCV and PoseLib end with, a Levenberg-Marquardt fit of the geometric error over the rows inside the threshold
(`refine_homography` / `refine_fundamental`, `roma_op_refine_model`, csrc/model_refine.hip; restated by tools/model_refine_ref.py).
method="magsac" (`magsac`, `roma_op_magsac`) keeps the sampling and scores each model by the MAGSAC++ loss (Barath et al.,
CVPR 2020, nu = 4) instead of its inlier count, then runs IRLS steps with the MAGSAC++ weights - what demo_fundamental asks
OpenCV for with USAC_MAGSAC, as the paper defines it (not OpenCV's implementation); restated by tools/magsac_ref.py.

Both models map A to B in pixel coordinates: x_B ~ H x_A and x_B^T F x_A = 0, like OpenCV's (points1 = A, points2 = B).  H and F
are scaled so that [2, 2] = 1 (unit Frobenius norm where |[2, 2]| < 1e-12 of it); F has rank 2.

The relative pose of the reference's pose benchmarks (romatch/utils/utils.py estimate_pose: cv2.findEssentialMat + cv2.recoverPose)
runs on the device as well (`roma_op_essential` / `roma_op_recover_pose`, csrc/essential.hip): `find_essential`, `recover_pose`,
`estimate_pose`, `estimate_pose_uncalibrated` and the five-point solver alone, `essential_minimal`.  Restated in numpy float64 by
tools/essential_ref.py.  method="magsac" there (`essential_magsac`, `roma_op_essential_magsac`) scores the five-point models by the
MAGSAC++ loss of their Sampson distance and optimises the winner over all the rows it weighs; restated by
tools/essential_magsac_ref.py.  `refine_pose` (`roma_op_refine_pose`, csrc/pose_refine.hip) fits the recovered pose to its inliers by
Levenberg-Marquardt on the truncated Sampson error, as the reference's PoseLib benchmark does; restated by tools/pose_refine_ref.py.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import _ptr, _stream

HOMOGRAPHY, FUNDAMENTAL = 0, 1
SAMPLE_SIZE = {HOMOGRAPHY: 4, FUNDAMENTAL: 7}
ROUND = 256  # hypotheses per pair and round (csrc/ransac.h RANSAC_ROUND)


def _as_batch(k: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(k, torch.Tensor) or not k.is_cuda:
        raise _lib.RomaHipError(f"roma_amd.geometry: {name} must be a tensor on a HIP device; there is no CPU fallback")
    if k.dim() not in (2, 3) or k.shape[-1] != 2:
        raise ValueError(f"roma_amd.geometry: {name} must be [N, 2] or [B, N, 2], got {tuple(k.shape)}")
    if k.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"roma_amd.geometry: {name} must be float32 or float64, got {k.dtype}")
    return k.detach().to(torch.float32).contiguous()


def _pair_batch(kpts_A, kpts_B):
    a, b = _as_batch(kpts_A, "kpts_A"), _as_batch(kpts_B, "kpts_B")
    a = a[None] if a.dim() == 2 else a
    b = b[None] if b.dim() == 2 else b
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"roma_amd.geometry: kpts_A {tuple(kpts_A.shape)} and kpts_B {tuple(kpts_B.shape)} differ in shape")
    if a.device != b.device:
        raise ValueError("roma_amd.geometry: kpts_A and kpts_B live on different devices")
    return a, b


def _cameras(camera_matrix, B, dev):
    """[B, 3, 3] float64 device camera matrices, or None (identity)"""
    if camera_matrix is None:
        return None
    K = torch.as_tensor(camera_matrix).to(device=dev, dtype=torch.float64)
    if K.shape == (3, 3):
        K = K[None].expand(B, 3, 3)
    if K.shape != (B, 3, 3):
        raise ValueError(f"roma_amd.geometry: camera_matrix must be [3, 3] or [{B}, 3, 3], got {tuple(K.shape)}")
    return K.contiguous()


def _counts(counts, B, dev):
    if counts is None:
        return None
    counts = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if counts.shape[0] != B:
        raise ValueError(f"roma_amd.geometry: counts has {counts.shape[0]} entries for {B} pairs")
    return counts


def _seeds(seed, B, dev):
    if seed is None:
        seeds = torch.randint(0, 2 ** 62, (B,), dtype=torch.int64)  # CPU generator: no device synchronisation
    elif isinstance(seed, torch.Tensor):
        seeds = seed.reshape(-1).to(torch.int64)
        if seeds.shape[0] != B:
            raise ValueError(f"roma_amd.geometry: {seeds.shape[0]} seeds for {B} pairs")
    else:
        seeds = torch.full((B,), int(seed), dtype=torch.int64)
    return seeds.to(dev).contiguous()  # read as uint64 by the kernels


def _single(kpts):
    """the single-pair form of the public functions: [N, 2] keypoints"""
    return isinstance(kpts, torch.Tensor) and kpts.dim() == 2


def _valid(valid, B, dev):
    if valid is None:
        return None
    valid = torch.as_tensor(valid).to(device=dev).reshape(-1).to(torch.uint8).contiguous()
    if valid.shape[0] != B:
        raise ValueError(f"roma_amd.geometry: valid has {valid.shape[0]} entries for {B} pairs")
    return valid


MAGSAC_MAX_LO = 64  # csrc/geometry.hip, csrc/essential.hip
# roma_op_<op>: (info columns, score columns, what the confidence argument is called)
ROBUST_OPS = {"ransac": (6, 0, "confidence"), "magsac": (7, 2, "confidence"), "essential": (5, 0, "prob"),
              "essential_magsac": (7, 2, "prob")}


def _robust(op, kpts_A, kpts_B, threshold, confidence, max_iters, seed, counts, option=None, model=None, camera_matrix=None):
    """ransac(), magsac(), essential() and essential_magsac(): the argument checks, zeroed outputs (M [B, 3, 3] float64, mask
    [B, N] bool, ok [B] bool, info int32, and score float64 where the op has one: ROBUST_OPS), counts and seeds on the device,
    then roma_op_<op>.  model: HOMOGRAPHY or FUNDAMENTAL, None for the essential matrix (which takes camera_matrix); option: the
    op's `refine` or `lo_iters`, None where it has neither.  Nothing is launched for B == 0 or fewer columns than a minimal
    sample, where no pair can hold one."""
    ninfo, nscore, conf_name = ROBUST_OPS[op]
    a, b = _pair_batch(kpts_A, kpts_B)
    if model is not None and model not in SAMPLE_SIZE:
        raise ValueError(f"roma_amd.geometry: unknown model {model}")
    if not (threshold > 0) or not (0 <= confidence <= 1) or int(max_iters) <= 0:
        raise ValueError(f"roma_amd.geometry: need threshold > 0, 0 <= {conf_name} <= 1, max_iters > 0")
    if nscore and not (0 <= int(option) <= MAGSAC_MAX_LO):
        raise ValueError(f"roma_amd.geometry: lo_iters must lie in [0, {MAGSAC_MAX_LO}]")
    B, N, dev = int(a.shape[0]), int(a.shape[1]), a.device
    outs = (torch.zeros((B, 3, 3), device=dev, dtype=torch.float64), torch.zeros((B, N), device=dev, dtype=torch.bool),
            torch.zeros((B,), device=dev, dtype=torch.bool), torch.zeros((B, ninfo), device=dev, dtype=torch.int32))
    if nscore:
        outs = outs + (torch.zeros((B, nscore), device=dev, dtype=torch.float64),)
    if B == 0:
        return outs
    counts, seeds = _counts(counts, B, dev), _seeds(seed, B, dev)
    # the tensors live until the launch is enqueued
    front = (a, b, counts, seeds, _cameras(camera_matrix, B, dev)) if model is None else (int(model), a, b, counts, seeds)
    if N < (5 if model is None else SAMPLE_SIZE[model]):
        return outs
    tail = (float(threshold), float(confidence), int(max_iters)) + (() if option is None else (int(option),))
    lib = _lib.load()
    nws = int(getattr(lib, f"roma_op_{op}_workspace")(B, N))
    ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, f"roma_op_{op}")(*(x if isinstance(x, int) else _ptr(x) for x in front), B, N, *tail,
                                                 *map(_ptr, outs), _ptr(ws), nws, _stream(dev)))
    return outs


def ransac(model: int, kpts_A: torch.Tensor, kpts_B: torch.Tensor, threshold: float, confidence: float, max_iters: int,
           seed=None, refine: bool = True, counts=None):
    """Batched robust estimation, no host synchronisation.  kpts [B, N, 2] device pixel coordinates; counts [B] rows per pair
    (rows at or beyond counts[b] are never read); seed an int (every pair), a [B] tensor (one per pair) or None (drawn from
    torch's CPU generator).  Returns (M [B, 3, 3] float64, mask [B, N] bool, ok [B] bool, info [B, 6] int32) with
    info = (rounds run, winning hypothesis, its root, its inlier count, final inlier count, pair valid)."""
    return _robust("ransac", kpts_A, kpts_B, threshold, confidence, max_iters, seed, counts, 1 if refine else 0, model=model)


def magsac(model: int, kpts_A: torch.Tensor, kpts_B: torch.Tensor, threshold: float, confidence: float, max_iters: int,
           seed=None, lo_iters: int = 10, counts=None):
    """Batched robust estimation with MAGSAC++ scoring (roma_op_magsac; Barath et al., CVPR 2020, nu = 4, as restated in
    tools/magsac_ref.py - not OpenCV's USAC_MAGSAC implementation), no host synchronisation.  The sampling of `ransac` (same
    samples, minimal solvers and adaptive iteration count), but each model is scored by the sum over the pair's rows of the
    MAGSAC++ loss of its pixel residual (H: reprojection error in image B; F: Sampson distance) and the smallest score wins; then
    up to lo_iters IRLS steps with the MAGSAC++ weights, each kept only if the score drops.  threshold is the largest residual
    that counts as an inlier (sigma_max = threshold / sqrt(13.2767), the 0.99 quantile of chi^2 with 4 DoF).

    Inputs as for `ransac`.  Returns (M [B, 3, 3] float64, mask [B, N] bool (residual < threshold), ok [B] bool,
    info [B, 7] int32, score [B, 2] float64) with info = (rounds run, winning hypothesis, its root, inliers of the winning minimal
    model, final inliers, pair valid, LO steps accepted) and score = (loss of the winning minimal model, final loss: that less the gains of the accepted LO steps)."""
    return _robust("magsac", kpts_A, kpts_B, threshold, confidence, max_iters, seed, counts, lo_iters, model=model)


def _method(method, plain=None, scored=None):
    """`plain` for method "ransac", `scored` for method "magsac"; any other method is an error"""
    if method not in ("ransac", "magsac"):
        raise ValueError(f"roma_amd.geometry: method must be 'ransac' or 'magsac', got {method!r}")
    return plain if method == "ransac" else scored


def _estimate(model, kpts_A, kpts_B, threshold, confidence, max_iters, seed, refine, counts, method):
    """(M, mask, ok) of `ransac` (method "ransac") or `magsac` (method "magsac"; refine=False means lo_iters=0)"""
    fn = _method(method, ransac, magsac)
    return fn(model, kpts_A, kpts_B, threshold, confidence, max_iters, seed, refine if fn is ransac else 10 if refine else 0, counts)[:3]


MODEL_MIN_ROWS = {HOMOGRAPHY: 4, FUNDAMENTAL: 7}  # csrc/model_refine.hip: rows below which nothing is fitted


def _refine(op, head, start, a, b, threshold, max_steps, counts, valid, min_rows, need, cost=False):
    """roma_op_refine_<op>(*head, *start, ...) on the pair batch a, b [B, N, 2]: (*fitted, mask [B, N] bool, info [B, 4] int32)
    and, if cost, cost [B, 2] float64.  start: the [B, r, c] float64 tensors to fit.  Nothing is launched for B == 0 or fewer
    than min_rows columns: every pair comes back untouched."""
    B, N, dev = int(a.shape[0]), int(a.shape[1]), a.device
    if not (threshold > 0) or int(max_steps) < 0:
        raise ValueError(f"roma_amd.geometry: need {need} > 0, max_steps >= 0")
    counts, valid = _counts(counts, B, dev), _valid(valid, B, dev)
    mask = torch.zeros((B, N), device=dev, dtype=torch.bool)
    info = torch.zeros((B, 4), device=dev, dtype=torch.int32)
    extra = (torch.full((B, 2), float("nan"), device=dev, dtype=torch.float64),) if cost else ()
    if B == 0 or N < min_rows:
        return (*(x.clone() for x in start), mask, info, *extra)
    out = tuple(torch.empty_like(x) for x in start)
    lib = _lib.load()
    nws = int(getattr(lib, f"roma_op_refine_{op}_workspace")(B, N))
    ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, f"roma_op_refine_{op}")(*head, *map(_ptr, start), _ptr(a), _ptr(b), _ptr(counts), _ptr(valid), B, N,
                                                        float(threshold), int(max_steps), *map(_ptr, out), _ptr(mask), _ptr(info),
                                                        *map(_ptr, extra), _ptr(ws), nws, _stream(dev)))
    return (*out, mask, info, *extra)


def _refine_model(model, M, kpts_A, kpts_B, threshold, max_steps, counts, valid, name):
    """roma_op_refine_model on [B, N, 2] pixels: (M [B, 3, 3] float64, mask [B, N] bool, info [B, 4] int32, cost [B, 2] float64)"""
    a, b = _pair_batch(kpts_A, kpts_B)
    M = _pose_tensor(M, name, int(a.shape[0]), (3, 3), a.device)
    return _refine("model", (int(model),), (M,), a, b, threshold, max_steps, counts, valid, MODEL_MIN_ROWS[model], "threshold", True)


def _refine_front(model, M, kpts_A, kpts_B, threshold, max_steps, counts, valid, name):
    out = _refine_model(model, M, kpts_A, kpts_B, threshold, max_steps, counts, valid, name)
    return tuple(o[0] for o in out) if _single(kpts_A) else out


def refine_homography(H, kpts_A, kpts_B, threshold, max_steps=25, counts=None, valid=None):
    """Nonlinear refinement of a homography on the device (roma_op_refine_model, csrc/model_refine.hip): a Levenberg-Marquardt
    fit of H to the forward reprojection error |H x_A - x_B| in image B under the truncated loss sum min(|e|^2, threshold^2) -
    the cost cv2.findHomography(..., cv2.RANSAC) ends with; restated in numpy float64 by tools/model_refine_ref.py.  The rows
    inside the threshold are re-evaluated with every cost (OpenCV freezes them to the RANSAC mask).  The fit runs in the
    Hartley-normalised coordinates of the pair; the largest entry of the normalised start is held fixed.  At most max_steps
    accepted steps; a fit that cannot move (fewer than 4 rows inside the threshold, a singular system) returns its input, so
    the truncated cost never rises and a model is never lost.  threshold in pixels; inf means plain least squares.

    H [3, 3] with kpts [N, 2] -> (H [3, 3] float64, mask [N] bool, info [4] int32, cost [2] float64);
    H [B, 3, 3] with kpts [B, N, 2] -> (H [B, 3, 3], mask [B, N], info [B, 4], cost [B, 2]).  No host synchronisation in either
    form.  H is scaled like find_homography's; mask: rows whose error is below threshold under the returned H;
    info = (accepted steps, cost evaluations, active rows at the end, pair fitted); cost = truncated cost in px^2 at (start,
    end), NaN where nothing was fitted.  valid [B] bool marks the pairs to fit; the others, and pairs of fewer than 4 rows,
    come back untouched with an empty mask and info[3] = 0.  See `ransac` for counts."""
    return _refine_front(HOMOGRAPHY, H, kpts_A, kpts_B, threshold, max_steps, counts, valid, "H")


def refine_fundamental(F, kpts_A, kpts_B, threshold, max_steps=25, counts=None, valid=None):
    """Nonlinear refinement of a fundamental matrix on the device (roma_op_refine_model): a Levenberg-Marquardt fit of F to the
    Sampson distance in pixels under the truncated loss sum min(r^2, threshold^2) - the cost PoseLib's estimate_fundamental ends
    with; restated by tools/model_refine_ref.py.  F = U diag(1, sigma, 0) V^T is updated on the rotations U, V and on sigma
    (seven parameters), so it has rank 2 at every iterate; a start of full rank is projected first.  Needs 7 rows inside the
    threshold.  Arguments and returns as `refine_homography`."""
    return _refine_front(FUNDAMENTAL, F, kpts_A, kpts_B, threshold, max_steps, counts, valid, "F")


def _polished(model, M, mask, ok, kpts_A, kpts_B, threshold, lm_steps, counts):
    """the lm_steps > 0 tail of find_*: pairs without a model are passed as not valid and keep what they had"""
    if int(lm_steps) < 0:
        raise ValueError("roma_amd.geometry: lm_steps must not be negative")
    if int(lm_steps) == 0:
        return M, mask
    return _refine_model(model, M, kpts_A, kpts_B, threshold, lm_steps, counts, ok, "model")[:2]


def _front(kpts_A, outs, ok, none):
    """what the public functions return: for a batch outs + (ok,); for a single pair ([N, 2] kpts) the first entry of each of
    outs, or `none` when no model was found - the one host synchronisation of the single-pair forms (OpenCV returns None)"""
    if not _single(kpts_A):
        return (*outs, ok)
    return tuple(o[0] for o in outs) if bool(ok[0]) else none


def find_homography(kpts_A, kpts_B, ransac_reproj_threshold=3.0, confidence=0.995, max_iters=2000, seed=None, refine=True,
                    counts=None, method="ransac", lm_steps=0):
    """cv2.findHomography(kpts_A, kpts_B, cv2.RANSAC, ransac_reproj_threshold, maxIters=max_iters, confidence=confidence) on the
    device: 4-point DLT hypotheses (OpenCV's checkSubset), inliers |H x_A - x_B| < threshold in image B.
    method="magsac": the same sampling with MAGSAC++ scoring and IRLS local optimisation (`magsac`; refine=False: lo_iters=0).
    lm_steps > 0: the model found, by either method, then goes through `refine_homography` (the call's threshold, at most
    lm_steps accepted steps; pairs without a model are left alone) - the Levenberg-Marquardt fit OpenCV ends with - and mask
    is the refinement's.  The default 0 leaves every output as it was before the keyword existed.

    kpts_A, kpts_B: [N, 2] -> (H [3, 3] float64, mask [N] bool) or (None, None) when no model was found;
    [B, N, 2] -> (H [B, 3, 3], mask [B, N], ok [B]) with no host synchronisation.  See `ransac` for seed and counts."""
    M, mask, ok = _estimate(HOMOGRAPHY, kpts_A, kpts_B, ransac_reproj_threshold, confidence, max_iters, seed, refine, counts,
                            method)
    M, mask = _polished(HOMOGRAPHY, M, mask, ok, kpts_A, kpts_B, ransac_reproj_threshold, lm_steps, counts)
    return _front(kpts_A, (M, mask), ok, (None, None))


def find_fundamental(kpts_A, kpts_B, ransac_reproj_threshold=3.0, confidence=0.99, max_iters=1000, seed=None, refine=True,
                     counts=None, method="ransac", lm_steps=0):
    """cv2.findFundamentalMat(kpts_A, kpts_B, cv2.FM_RANSAC, ransac_reproj_threshold, confidence, max_iters) on the device:
    7-point hypotheses (up to 3 models each), inliers whose distances to both epipolar lines are below the threshold.
    method="magsac": the same sampling with MAGSAC++ scoring of the Sampson distance and IRLS local optimisation (`magsac`;
    refine=False: lo_iters=0) - what demo_fundamental's cv2.USAC_MAGSAC call asks for, as MAGSAC++ is defined in the paper.
    lm_steps > 0: the model found, by either method, then goes through `refine_fundamental` (the call's threshold on the Sampson
    distance, at most lm_steps accepted steps; pairs without a model are left alone) and mask is the refinement's.  The default
    0 leaves every output as it was before the keyword existed.

    kpts_A, kpts_B: [N, 2] -> (F [3, 3] float64, mask [N] bool) or (None, None) when no model was found;
    [B, N, 2] -> (F [B, 3, 3], mask [B, N], ok [B]) with no host synchronisation.  See `ransac` for seed and counts."""
    M, mask, ok = _estimate(FUNDAMENTAL, kpts_A, kpts_B, ransac_reproj_threshold, confidence, max_iters, seed, refine, counts,
                            method)
    M, mask = _polished(FUNDAMENTAL, M, mask, ok, kpts_A, kpts_B, ransac_reproj_threshold, lm_steps, counts)
    return _front(kpts_A, (M, mask), ok, (None, None))


# ---------------------------------------------------------------------------------------------------- essential matrix and pose
ESSENTIAL_MAX_ROOTS = 10  # solutions of one five-point sample (csrc/essential.hip)


def essential(kpts_A, kpts_B, camera_matrix=None, prob=0.999, threshold=1.0, max_iters=1000, seed=None, counts=None):
    """Batched cv2.findEssentialMat, no host synchronisation.  Returns (E [B, 3, 3] float64, mask [B, N] bool, ok [B] bool,
    info [B, 5] int32) with info = (rounds run, winning hypothesis, its root, inlier count, pair valid)."""
    return _robust("essential", kpts_A, kpts_B, threshold, prob, max_iters, seed, counts, camera_matrix=camera_matrix)


def essential_magsac(kpts_A, kpts_B, camera_matrix=None, prob=0.999, threshold=1.0, max_iters=1000, seed=None, lo_iters=10,
                     counts=None):
    """`essential` with MAGSAC++ scoring and local optimisation (roma_op_essential_magsac; Barath et al., CVPR 2020, nu = 4, as
    restated in tools/essential_magsac_ref.py), no host synchronisation.  The sampling of `essential` (same samples, five-point
    models and adaptive iteration count), but each model is scored by the sum over the pair's rows of the MAGSAC++ loss of its
    Sampson distance in normalised camera coordinates and the smallest score wins; then up to lo_iters IRLS steps - the
    MAGSAC++ weights of the current model, the weighted eight-point system over the rows of positive weight (at least 8), the
    five-point solver's cubic constraints on its four smallest eigenvectors - each kept only if the score drops.  threshold
    (divided by (fx + fy) / 2 under a camera matrix) is the largest residual that counts as an inlier.  lo_iters=0 returns the
    winning five-point model untouched.

    Inputs as for `essential`.  Returns (E [B, 3, 3] float64 on the essential manifold, unit norm, largest-magnitude entry
    positive; mask [B, N] bool (residual < threshold: `essential`'s inlier rule); ok [B] bool; info [B, 7] int32; score [B, 2]
    float64) with info = (rounds run, winning hypothesis, its root, inliers of the winning minimal model, final inliers, pair
    valid, LO steps accepted) and score = (loss of the winning minimal model, final loss)."""
    return _robust("essential_magsac", kpts_A, kpts_B, threshold, prob, max_iters, seed, counts, lo_iters, camera_matrix=camera_matrix)


def _essential(kpts_A, kpts_B, camera_matrix, prob, threshold, max_iters, seed, counts, method, lo_iters):
    """(E, mask, ok) of `essential` (method "ransac") or `essential_magsac` (method "magsac")"""
    fn = _method(method, essential, essential_magsac)
    return fn(kpts_A, kpts_B, camera_matrix, prob, threshold, max_iters, seed, *(() if fn is essential else (lo_iters,)), counts)[:3]


def find_essential(kpts_A, kpts_B, camera_matrix=None, prob=0.999, threshold=1.0, max_iters=1000, seed=None, counts=None,
                   method="ransac", lo_iters=10):
    """cv2.findEssentialMat(kpts_A, kpts_B, camera_matrix, cv2.RANSAC, prob, threshold, max_iters) on the device: Nister's
    five-point hypotheses (up to 10 models each), inliers whose Sampson distance is below the threshold, no refinement.
    method="magsac": the same sampling with MAGSAC++ scoring and up to lo_iters steps of local optimisation
    (`essential_magsac`); lo_iters is not read otherwise.  The defaults leave every output as it was before the keywords existed.
    camera_matrix None means identity (the points are normalised already, as the reference calls it); a [3, 3] or [B, 3, 3]
    matrix normalises x_n = ((x - cx) / fx, (y - cy) / fy) and divides the threshold by (fx + fy) / 2, like OpenCV.  E relates
    the normalised points (x_B^T E x_A = 0), has unit Frobenius norm and its largest-magnitude entry positive.

    kpts_A, kpts_B: [N, 2] -> (E [3, 3] float64, mask [N] bool) or (None, None) when no model was found;
    [B, N, 2] -> (E [B, 3, 3], mask [B, N], ok [B]) with no host synchronisation.  See `ransac` for seed and counts."""
    E, mask, ok = _essential(kpts_A, kpts_B, camera_matrix, prob, threshold, max_iters, seed, counts, method, lo_iters)
    return _front(kpts_A, (E, mask), ok, (None, None))


def recover_pose(E, kpts_A, kpts_B, mask=None, camera_matrix=None, distance_thresh=1e9, counts=None):
    """cv2.recoverPose(E, kpts_A, kpts_B, camera_matrix, distance_thresh, mask) on the device.  The four decompositions
    (R1, t), (R2, t), (R1, -t), (R2, -t) of E (SVD with OpenCV's det(U), det(V^T) > 0 fix-up, t = U[:, 2]; E need not be exactly
    essential), linear triangulation of the masked rows, a row is good for a candidate if its depth is positive and below
    distance_thresh in both cameras; the candidate with the most good rows wins, ties to the earlier one.

    E [3, 3] with kpts [N, 2] -> (n_good int, R [3, 3] float64, t [3, 1] float64, mask_good [N] bool);
    E [B, 3, 3] with kpts [B, N, 2] -> (n_good [B] int32, R [B, 3, 3], t [B, 3, 1], mask_good [B, N]), no synchronisation."""
    a, b = _pair_batch(kpts_A, kpts_B)
    B, N, dev = int(a.shape[0]), int(a.shape[1]), a.device
    if not isinstance(E, torch.Tensor) or not E.is_cuda:
        raise _lib.RomaHipError("roma_amd.geometry: E must be a tensor on a HIP device; there is no CPU fallback")
    E = E.detach().to(device=dev, dtype=torch.float64).reshape(-1, 3, 3).contiguous()
    if E.shape[0] != B:
        raise ValueError(f"roma_amd.geometry: {E.shape[0]} matrices E for {B} pairs")
    if not (distance_thresh > 0):
        raise ValueError("roma_amd.geometry: distance_thresh must be positive")
    if mask is not None:
        mask = torch.as_tensor(mask).to(device=dev).reshape(B, N).to(torch.uint8).contiguous()
    K, counts = _cameras(camera_matrix, B, dev), _counts(counts, B, dev)
    n_good = torch.zeros((B,), device=dev, dtype=torch.int32)
    R = torch.zeros((B, 3, 3), device=dev, dtype=torch.float64)
    t = torch.zeros((B, 3, 1), device=dev, dtype=torch.float64)
    good = torch.zeros((B, N), device=dev, dtype=torch.bool)
    if B > 0 and N > 0:
        lib = _lib.load()
        nws = int(lib.roma_op_recover_pose_workspace(B, N))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_recover_pose(_ptr(E), _ptr(a), _ptr(b), _ptr(mask), _ptr(counts), _ptr(K), B, N,
                                                float(distance_thresh), _ptr(n_good), _ptr(R), _ptr(t), _ptr(good), _ptr(ws), nws,
                                                _stream(dev)))
    if _single(kpts_A):
        return int(n_good[0]), R[0], t[0], good[0]
    return n_good, R, t, good


def essential_minimal(x0, x1):
    """The five-point solver alone on caller-chosen samples: x0, x1 [S, 5, 2] normalised points (x1^T E x0 = 0) ->
    (E [S, 10, 3, 3] float64, n [S] int32); solution r < n[s] of sample s is E[s, r], in ascending order of Nister's z, unit
    Frobenius norm, largest-magnitude entry positive; unused slots are zero."""
    for name, x in (("x0", x0), ("x1", x1)):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.RomaHipError(f"roma_amd.geometry: {name} must be a tensor on a HIP device; there is no CPU fallback")
        if x.dim() != 3 or tuple(x.shape[1:]) != (5, 2):
            raise ValueError(f"roma_amd.geometry: {name} must be [S, 5, 2], got {tuple(x.shape)}")
    if x0.shape != x1.shape:
        raise ValueError("roma_amd.geometry: x0 and x1 differ in shape")
    S, dev = int(x0.shape[0]), x0.device
    a = x0.detach().to(torch.float64).contiguous()
    b = x1.detach().to(device=dev, dtype=torch.float64).contiguous()
    E = torch.zeros((S, ESSENTIAL_MAX_ROOTS, 3, 3), device=dev, dtype=torch.float64)
    n = torch.zeros((S,), device=dev, dtype=torch.int32)
    if S > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_essential_minimal(_ptr(a), _ptr(b), S, _ptr(E), _ptr(n),
                                                             _stream(dev)))
    return E, n


def _normalise_pose_points(kpts, K):
    """the reference's normalisation (utils.py:38-39): inverse of K[:2, :2] (skew included) after the principal point, f64"""
    k = kpts.to(torch.float64) - K[:, None, :2, 2]
    a, b, c, d = K[:, 0, 0, None], K[:, 0, 1, None], K[:, 1, 0, None], K[:, 1, 1, None]
    det = a * d - b * c  # closed-form 2 x 2 inverse: torch.linalg.inv would read its error flag back to the host
    return torch.stack(((d * k[..., 0] - b * k[..., 1]) / det, (a * k[..., 1] - c * k[..., 0]) / det), dim=-1)


def _pose_inputs(kpts0, kpts1, K0, K1, counts):
    a, b = _pair_batch(kpts0, kpts1)
    B, dev = int(a.shape[0]), a.device
    K0, K1 = _cameras(K0, B, dev), _cameras(K1, B, dev)
    if K0 is None or K1 is None:
        raise ValueError("roma_amd.geometry: K0 and K1 are required")
    return a, b, K0, K1, _counts(counts, B, dev)


def _pose_tensor(x, name, B, shape, dev):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.RomaHipError(f"roma_amd.geometry: {name} must be a tensor on a HIP device; there is no CPU fallback")
    x = x.detach().to(device=dev, dtype=torch.float64)
    if x.numel() != B * shape[0] * shape[1]:
        raise ValueError(f"roma_amd.geometry: {name} must hold {B} x {shape}, got {tuple(x.shape)}")
    return x.reshape(B, *shape).contiguous()


def _refine_normalised(R, t, x0, x1, thr, max_steps, counts, valid):
    """roma_op_refine_pose on normalised points [B, N, 2] (read as f32): (R [B, 3, 3], t [B, 3, 1], mask [B, N] bool,
    info [B, 4] int32)"""
    a, b = _pair_batch(x0, x1)
    B, dev = int(a.shape[0]), a.device
    start = (_pose_tensor(R, "R", B, (3, 3), dev), _pose_tensor(t, "t", B, (3, 1), dev))
    return _refine("pose", (), start, a, b, thr, max_steps, counts, valid, 5, "norm_thresh")


def refine_pose(R, t, kpts0, kpts1, K0, K1, norm_thresh, max_steps=25, counts=None, valid=None):
    """Nonlinear refinement of a relative pose on the device (roma_op_refine_pose, csrc/pose_refine.hip): a Levenberg-Marquardt
    fit of (R, t) to the Sampson error of E = [t]x R under the truncated loss sum min(r^2, norm_thresh^2) - what the final
    refinement of poselib.estimate_relative_pose is (the reference's megadepth_pose_estimation_benchmark_poselib.py); restated
    in numpy float64 by tools/pose_refine_ref.py.  The pixel keypoints are normalised as in estimate_pose; norm_thresh is the
    threshold estimate_pose takes.  At most max_steps accepted steps; a fit that cannot move (no or fewer than 5 rows inside
    the threshold, a singular system) returns its input, so the truncated cost never rises and a pose is never lost.

    R [3, 3], t [3, 1] with kpts [N, 2] -> (R [3, 3] float64, t [3, 1] float64, mask [N] bool, info [4] int32);
    R [B, 3, 3], t [B, 3, 1] with kpts [B, N, 2] -> (R [B, 3, 3], t [B, 3, 1], mask [B, N], info [B, 4]).  No host
    synchronisation in either form.  mask: rows whose Sampson error is below norm_thresh under the returned pose and whose
    depth is positive in both cameras (the triangulation of recover_pose); info = (accepted steps, cost evaluations, active
    rows at the end, pair fitted).  valid [B] bool marks the pairs to fit; the others, and pairs of fewer than 5 rows, come
    back untouched with an empty mask and info[3] = 0.  See `ransac` for counts."""
    a, b, K0, K1, counts = _pose_inputs(kpts0, kpts1, K0, K1, counts)
    x0, x1 = _normalise_pose_points(a, K0), _normalise_pose_points(b, K1)
    out = _refine_normalised(R, t, x0, x1, norm_thresh, max_steps, counts, valid)
    return tuple(o[0] for o in out) if _single(kpts0) else out


def _refined(R, t, good, ok, x0, x1, thr, counts):
    """the refine=True tail of estimate_pose*: pairs without a pose are passed as not valid and keep what they had"""
    R, t, mask, info = _refine_normalised(R, t, x0, x1, thr, 25, counts, ok)
    return R, t, torch.where(info[:, 3:4] > 0, mask, good)


def estimate_pose(kpts0, kpts1, K0, K1, norm_thresh, conf=0.99999, max_iters=1000, seed=None, counts=None, refine=False,
                  method="ransac"):
    """romatch/utils/utils.py:30-51 on the device: normalise with the inverse of K[:2, :2] and the principal point (f64), then
    find_essential (identity camera, threshold norm_thresh, prob conf) and recover_pose.

    [N, 2] -> (R [3, 3], t [3, 1], mask [N] bool) or None (also for fewer than 5 rows); [B, N, 2] -> (R [B, 3, 3],
    t [B, 3, 1], mask [B, N], ok [B]) with no host synchronisation.  mask is what the reference returns: cv2.recoverPose rewrites the RANSAC mask in place, so it holds
    the RANSAC inliers that pass the cheirality test of the chosen candidate (tools/pose_geometry.estimate_pose returns the plain
    RANSAC mask instead).

    refine=True: the recovered pose, which is the winning five-point sample's, then goes through `refine_pose` (threshold
    norm_thresh, 25 steps; pairs without a pose are left alone) and mask is the refined one.  The default leaves every output
    as it was before the keyword existed.

    method="magsac": E comes from `essential_magsac` (MAGSAC++ scoring, 10 steps of local optimisation over all the rows it
    weighs) instead of `essential`; recover_pose and refine=True follow as above.  The default "ransac" leaves every output as
    it was before the keyword existed."""
    _method(method)
    a, b, K0, K1, counts = _pose_inputs(kpts0, kpts1, K0, K1, counts)
    x0, x1 = _normalise_pose_points(a, K0), _normalise_pose_points(b, K1)
    E, inl, ok = _essential(x0, x1, None, conf, norm_thresh, max_iters, seed, counts, method, 10)
    n, R, t, good = recover_pose(E, x0, x1, inl, None, 1e9, counts)
    ok = ok & (n > 0)
    if refine:
        R, t, good = _refined(R, t, good, ok, x0, x1, norm_thresh, counts)
    return _front(kpts0, (R, t, good), ok, None)


def _mean_focal(K0, K1):
    """mean of fx, fy of both cameras as a Python float; host arithmetic when the matrices were given on the host"""
    f = [torch.as_tensor(K).to(torch.float64).reshape(-1, 3, 3)[:, (0, 1), (0, 1)].mean() for K in (K0, K1)]
    return 0.5 * (float(f[0]) + float(f[1]))


def estimate_pose_uncalibrated(kpts0, kpts1, K0, K1, norm_thresh, conf=0.99999, max_iters=10000, seed=None, counts=None,
                               refine=False, method="ransac"):
    """romatch/utils/utils.py:53-74 on the device: find_fundamental on the pixels (threshold norm_thresh in pixels, as the
    reference passes it; plain RANSAC + LO standing in for USAC_ACCURATE), E = K1^T F K0, then recover_pose on the normalised
    points.  Returns as estimate_pose.

    refine=True: as in estimate_pose.  The refinement works on normalised points, so it gets norm_thresh divided by the mean of
    the four focal lengths (fx, fy of K0 and of K1; over all pairs where the matrices are [B, 3, 3]).  That mean is a host
    number: camera matrices given on the host (numpy, CPU tensors) cost nothing, matrices that live on the device are read back
    once, which is the one host synchronisation of this option.

    method="magsac": F comes from `magsac` (MAGSAC++ scoring and IRLS local optimisation, lo_iters 10) instead of `ransac` - the
    USAC-style estimator the reference asks OpenCV for.  The default "ransac" leaves every output as it was before the keyword
    existed."""
    _method(method)
    focal = _mean_focal(K0, K1) if refine else None
    a, b, K0, K1, counts = _pose_inputs(kpts0, kpts1, K0, K1, counts)
    F, inl, ok = _estimate(FUNDAMENTAL, a, b, norm_thresh, conf, max_iters, seed, True, counts, method)
    E = K1.transpose(1, 2) @ F @ K0
    x0, x1 = _normalise_pose_points(a, K0), _normalise_pose_points(b, K1)
    n, R, t, good = recover_pose(E, x0, x1, inl, None, 1e9, counts)
    ok = ok & (n > 0)
    if refine:
        R, t, good = _refined(R, t, good, ok, x0, x1, norm_thresh / focal, counts)
    return _front(kpts0, (R, t, good), ok, None)
