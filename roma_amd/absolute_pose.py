"""Absolute pose on the device (`roma_op_absolute_pose`, csrc/absolute_pose.hip): the pose of a camera from rows of a 3-D point
and its image - the second thing a dense matcher's output is used for, after relative pose.  Visual localisation: a query
image matched against a database image that has depth (`lift_matches`, then `estimate_absolute_pose`; or
`RegressionMatcher.localize`).  Incremental reconstruction: A and B triangulated with `triangulate_warp`, then C registered
against A's points.  Batched over pairs, no read-back: the points come from `triangulate` / a depth map, the matches from
`sample_batched` / `match_keypoints_batched`, and both stay on the device.

P3P RANSAC (samples of three rows, up to four poses each, inlier = positive depth and reprojection error below the threshold,
OpenCV's adaptive iteration count) followed by a Levenberg-Marquardt fit of the reprojection error under a truncated loss
(`refine_absolute_pose`).  The algorithm is restated in numpy float64 by tools/absolute_pose_ref.py.  x_cam = R X + t.
"""
from __future__ import annotations

from functools import partial

import torch

from . import _lib
from ._lib import _ptr, _stream
from .geometry import _cameras, _counts, _front, _pose_tensor, _seeds, _valid

SLOTS = 4  # solutions of one P3P sample (csrc/absolute_pose.hip AP_SLOTS)


_device_tensor = partial(_lib._device_tensor, module="absolute_pose")


def _rows(points3d, kpts):
    """([B, N, 3] f32, [B, N, 2] f32) of the single-pair or batched inputs"""
    X, x = _device_tensor(points3d, "points3d"), _device_tensor(kpts, "kpts")
    for t, name, c in ((X, "points3d", 3), (x, "kpts", 2)):
        if t.dim() not in (2, 3) or t.shape[-1] != c:
            raise ValueError(f"roma_amd.absolute_pose: {name} must be [N, {c}] or [B, N, {c}], got {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"roma_amd.absolute_pose: {name} must be float32 or float64, got {t.dtype}")
    X = X.detach().to(torch.float32).contiguous()
    x = x.detach().to(device=X.device, dtype=torch.float32).contiguous()
    X = X[None] if X.dim() == 2 else X
    x = x[None] if x.dim() == 2 else x
    if X.shape[:2] != x.shape[:2]:
        raise ValueError(f"roma_amd.absolute_pose: points3d {tuple(points3d.shape)} and kpts {tuple(kpts.shape)} differ in rows")
    return X, x


def absolute_pose(points3d, kpts, K=None, reproj_thresh=2.0, conf=0.9999, max_iters=1000, seed=None, counts=None):
    """Batched P3P RANSAC (roma_op_absolute_pose), no host synchronisation and no refinement.  points3d [B, N, 3], kpts
    [B, N, 2] on the device; K, counts and seed as for `estimate_absolute_pose`.  Returns (R [B, 3, 3] float64, t [B, 3, 1]
    float64, mask [B, N] bool, ok [B] bool, info [B, 5] int32) with info = (rounds run, winning hypothesis, its slot, its inlier
    count, pair valid)."""
    X, x = _rows(points3d, kpts)
    if not (reproj_thresh > 0) or not (0 <= conf <= 1) or int(max_iters) <= 0:
        raise ValueError("roma_amd.absolute_pose: need reproj_thresh > 0, 0 <= conf <= 1, max_iters > 0")
    B, N, dev = int(X.shape[0]), int(X.shape[1]), X.device
    R = torch.zeros((B, 3, 3), device=dev, dtype=torch.float64)
    t = torch.zeros((B, 3, 1), device=dev, dtype=torch.float64)
    mask = torch.zeros((B, N), device=dev, dtype=torch.bool)
    ok = torch.zeros((B,), device=dev, dtype=torch.bool)
    info = torch.zeros((B, 5), device=dev, dtype=torch.int32)
    if B == 0 or N < 4:  # no pair can hold four rows
        return R, t, mask, ok, info
    K, counts, seeds = _cameras(K, B, dev), _counts(counts, B, dev), _seeds(seed, B, dev)
    lib = _lib.load()
    nws = int(lib.roma_op_absolute_pose_workspace(B, N))
    ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(lib.roma_op_absolute_pose(_ptr(X), _ptr(x), _ptr(counts), _ptr(seeds), _ptr(K), B, N, float(reproj_thresh),
                                             float(conf), int(max_iters), _ptr(R), _ptr(t), _ptr(mask), _ptr(ok), _ptr(info),
                                             _ptr(ws), nws, _stream(dev)))
    return R, t, mask, ok, info


def _refine(R, t, X, x, K, reproj_thresh, max_steps, counts, valid):
    """roma_op_refine_absolute_pose on [B, N, 3] / [B, N, 2] f32 rows: (R [B, 3, 3], t [B, 3, 1], mask [B, N] bool, info [B, 4])"""
    B, N, dev = int(X.shape[0]), int(X.shape[1]), X.device
    if not (reproj_thresh > 0) or int(max_steps) < 0:
        raise ValueError("roma_amd.absolute_pose: need reproj_thresh > 0, max_steps >= 0")
    R, t = _pose_tensor(R, "R", B, (3, 3), dev), _pose_tensor(t, "t", B, (3, 1), dev)
    K, counts, valid = _cameras(K, B, dev), _counts(counts, B, dev), _valid(valid, B, dev)
    mask = torch.zeros((B, N), device=dev, dtype=torch.bool)
    info = torch.zeros((B, 4), device=dev, dtype=torch.int32)
    if B == 0 or N < 3:
        return R.clone(), t.clone(), mask, info
    out_r, out_t = torch.empty_like(R), torch.empty_like(t)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().roma_op_refine_absolute_pose(_ptr(R), _ptr(t), _ptr(X), _ptr(x), _ptr(counts), _ptr(valid), _ptr(K), B,
                                                            N, float(reproj_thresh), int(max_steps), _ptr(out_r), _ptr(out_t),
                                                            _ptr(mask), _ptr(info), _stream(dev)))
    return out_r, out_t, mask, info


def refine_absolute_pose(R, t, points3d, kpts, K, reproj_thresh, max_steps=25, counts=None, valid=None):
    """Nonlinear refinement of an absolute pose on the device (roma_op_refine_absolute_pose): a Levenberg-Marquardt fit of (R, t)
    to the reprojection error under the truncated loss sum min(|r|^2, reproj_thresh^2), on the normalised problem
    `estimate_absolute_pose` solves (image points through K, 3-D points centred and scaled); restated by
    tools/absolute_pose_ref.py.  A row whose depth is not positive or that holds a non-finite value takes no part.  At most
    max_steps accepted steps; a fit that cannot move (fewer than 3 rows inside the threshold, a singular system) returns its
    input, so the truncated cost never rises and a pose is never lost.  K None: kpts are normalised image coordinates and so is
    the threshold.

    R [3, 3], t [3, 1] with points3d [N, 3], kpts [N, 2] -> (R [3, 3] float64, t [3, 1] float64, mask [N] bool, info [4] int32);
    R [B, 3, 3], t [B, 3, 1] with [B, N, 3], [B, N, 2] -> (R [B, 3, 3], t [B, 3, 1], mask [B, N], info [B, 4]).  No host
    synchronisation in either form.  mask: the rows inside the threshold under the returned pose; info = (accepted steps, cost
    evaluations, active rows at the end, pair fitted).  valid [B] bool marks the pairs to fit; the others, and pairs of fewer
    than 4 finite rows, come back untouched with an empty mask and info[3] = 0.  See `ransac` for counts."""
    X, x = _rows(points3d, kpts)
    out = _refine(R, t, X, x, K, reproj_thresh, max_steps, counts, valid)
    return tuple(o[0] for o in out) if points3d.dim() == 2 else out


def estimate_absolute_pose(points3d, kpts, K=None, reproj_thresh=2.0, conf=0.9999, max_iters=1000, seed=None, counts=None,
                           refine=True, max_steps=25):
    """The pose (R, t), x_cam = R X + t, of the camera that sees the 3-D points points3d at the pixels kpts: P3P RANSAC
    (`absolute_pose`), then refine=True `refine_absolute_pose` from the winning sample's pose (threshold reproj_thresh, at most
    max_steps steps; pairs without a pose are left alone).  K: [3, 3] or [B, 3, 3] camera matrix of kpts, applied by fx, fy, cx,
    cy; reproj_thresh is in its pixels (divided by (fx + fy) / 2, as `find_essential` does).  K None: kpts are normalised image
    coordinates, and so is the threshold.  The 3-D points may lie anywhere: they are centred and scaled before the f32 scoring.
    A row with a non-finite entry (what `lift_matches` writes where there is no depth) is never an inlier and never sampled.

    points3d [N, 3], kpts [N, 2] -> (R [3, 3] float64, t [3, 1] float64, mask [N] bool), or None when no pose was found (fewer
    than 4 finite rows, all points one point, no model with 4 inliers); [B, N, 3], [B, N, 2] -> (R [B, 3, 3], t [B, 3, 1],
    mask [B, N], ok [B]) with no host synchronisation.  With refine=True mask is that of the refined pose.  See `ransac` for
    seed and counts."""
    X, x = _rows(points3d, kpts)
    R, t, mask, ok, _ = absolute_pose(X, x, K, reproj_thresh, conf, max_iters, seed, counts)
    if refine:
        R, t, fitted, info = _refine(R, t, X, x, K, reproj_thresh, max_steps, counts, ok)
        mask = torch.where(info[:, 3:4] > 0, fitted, mask)
    return _front(kpts, (R, t, mask), ok, None)


def absolute_pose_minimal(X, x):
    """The P3P solver alone on caller-chosen samples: X [S, 3, 3] points, x [S, 3, 2] normalised image points -> (R [S, 4, 3, 3]
    float64, t [S, 4, 3] float64, n [S] int32); solution r < n[s] of sample s is (R[s, r], t[s, r]): every real solution with
    three positive depths, in ascending order of the solver's root; unused slots are zero."""
    for name, v, c in (("X", X, 3), ("x", x, 2)):
        _device_tensor(v, name)
        if v.dim() != 3 or tuple(v.shape[1:]) != (3, c):
            raise ValueError(f"roma_amd.absolute_pose: {name} must be [S, 3, {c}], got {tuple(v.shape)}")
    if X.shape[0] != x.shape[0]:
        raise ValueError("roma_amd.absolute_pose: X and x differ in the number of samples")
    S, dev = int(X.shape[0]), X.device
    a = X.detach().to(torch.float64).contiguous()
    b = x.detach().to(device=dev, dtype=torch.float64).contiguous()
    R = torch.zeros((S, SLOTS, 3, 3), device=dev, dtype=torch.float64)
    t = torch.zeros((S, SLOTS, 3), device=dev, dtype=torch.float64)
    n = torch.zeros((S,), device=dev, dtype=torch.int32)
    if S > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_absolute_pose_minimal(_ptr(a), _ptr(b), S, _ptr(R), _ptr(t), _ptr(n), _stream(dev)))
    return R, t, n


def lift_matches(matches, depth_A, K_A, H_B, W_B):
    """Matches to the rows `estimate_absolute_pose` takes, through a depth map of image A (roma_op_lift_matches).  matches
    [N, 4] or [B, N, 4] in normalised coordinates as `sample_batched` returns them (columns 0:2 in A, 2:4 in B); depth_A [H, W]
    or [B, H, W]; K_A [3, 3] or [B, 3, 3], the camera of A at the depth map's size.  Returns (points3d [.., N, 3] float32 in
    camera A's frame, kpts_B [.., N, 2] float32 in pixels of an (H_B, W_B) image).  Depth is bilinear (align_corners=False) from
    four neighbours that are all finite and positive (`depth_consistency`'s rule); otherwise the row's point is NaN, which the
    pose kernels ignore - no compaction and no host read."""
    m, d = _device_tensor(matches, "matches"), _device_tensor(depth_A, "depth_A")
    if m.dim() not in (2, 3) or m.shape[-1] != 4:
        raise ValueError(f"roma_amd.absolute_pose: matches must be [N, 4] or [B, N, 4], got {tuple(m.shape)}")
    single = m.dim() == 2
    m = m.detach().to(torch.float32).contiguous()
    m = m[None] if single else m
    d = d.detach().to(device=m.device, dtype=torch.float32).contiguous()
    d = d[None] if d.dim() == 2 else d
    B, N, dev = int(m.shape[0]), int(m.shape[1]), m.device
    if d.dim() != 3 or d.shape[0] != B:
        raise ValueError(f"roma_amd.absolute_pose: depth_A must be [H, W] or [{B}, H, W], got {tuple(depth_A.shape)}")
    H, W = int(d.shape[1]), int(d.shape[2])
    if H <= 0 or W <= 0 or int(H_B) <= 0 or int(W_B) <= 0:
        raise ValueError("roma_amd.absolute_pose: image sizes must be positive")
    K = _cameras(K_A, B, dev)
    if K is None:
        raise ValueError("roma_amd.absolute_pose: K_A is required")
    pts = torch.empty((B, N, 3), device=dev, dtype=torch.float32)
    kb = torch.empty((B, N, 2), device=dev, dtype=torch.float32)
    if B > 0 and N > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_lift_matches(_ptr(m), _ptr(d), _ptr(K), B, N, H, W, int(H_B), int(W_B), _ptr(pts), _ptr(kb),
                                                        _stream(dev)))
    return (pts[0], kb[0]) if single else (pts, kb)
