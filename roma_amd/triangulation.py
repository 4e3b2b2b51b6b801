"""Triangulation on the device (`roma_op_triangulate`, `roma_op_depth_consistency`, csrc/triangulate.hip): the depth of every match
and its 3-D point from a warp (or sampled matches) and the relative pose the geometry functions return - the link after
`estimate_pose` / `refine_pose` in the chain match() -> sample_batched() -> estimate_pose().

The error model is a dense matcher's: the pixel on the grid of the reference image is exact, the predicted coordinate in the other
image carries the error, so the point lies on the reference pixel's ray at the depth whose projection into the other image is
closest to the prediction.  The two halves of a symmetric warp triangulate the same surface from both sides and can check each
other (`depth_consistency`: the reference's warp_kpts rule with triangulated depth in place of sensor depth).  The definition is
stated in include/roma_hip.h and restated in numpy float64 by tools/triangulate_ref.py.

Conventions are those of `roma_amd.geometry`: device tensors only, (R, t) maps camera A's frame to camera B's, cameras are applied
by fx, fy, cx, cy, no call synchronises with the host."""
from __future__ import annotations

import math
from collections import namedtuple
from functools import partial

import torch

from . import _lib
from ._lib import _ptr, _stream
from .geometry import _cameras, _counts, _pair_batch, _pose_tensor, _valid

SKIPPED, DEGENERATE, CHEIRALITY, REPROJ, PARALLAX, CERTAINTY = 1, 2, 4, 8, 16, 32  # bits of `flags` (csrc/triangulate.h)

Triangulation = namedtuple("Triangulation", "points depth_other reproj parallax flags valid stats")
ViewsTriangulation = namedtuple("ViewsTriangulation", "points reproj used parallax flags valid stats")
MAX_VIEWS = 8   # csrc/tracks.h: ROMA_TRACKS_MAX_VIEWS
MAX_GN = 10     # csrc/triangulate_views.hip: TRIANGULATE_VIEWS_MAX_GN


class WarpTriangulation(dict):
    """what `triangulate_warp` returns: a dict whose entries are also attributes"""
    __getattr__ = dict.__getitem__


_device_tensor = partial(_lib._device_tensor, module="triangulation")


def _thresholds(max_depth, max_reproj, min_parallax, min_certainty):
    th = tuple(float(x) for x in (max_depth, max_reproj, min_parallax, min_certainty))
    if not all(x >= 0 for x in th):
        raise ValueError("roma_amd.triangulation: max_depth, max_reproj, min_parallax and min_certainty must not be negative")
    return th


def _launch(m, certainty, R, t, K_A, K_B, counts, valid, coords, sizes, sym_w, thresholds):
    """roma_op_triangulate on matches [B, n, 4] float32 contiguous: Triangulation with the batch axis"""
    B, n, dev = int(m.shape[0]), int(m.shape[1]), m.device
    if B * n >= 2 ** 31 or B > 65535:
        raise ValueError(f"roma_amd.triangulation: {B} x {n} points is more than one call takes (B <= 65535, B n < 2^31)")
    R, t = _pose_tensor(R, "R", B, (3, 3), dev), _pose_tensor(t, "t", B, (3, 1), dev).reshape(B, 3)
    K_A, K_B = _cameras(K_A, B, dev), _cameras(K_B, B, dev)
    counts, valid = _counts(counts, B, dev), _valid(valid, B, dev)
    if certainty is not None:
        certainty = _device_tensor(certainty, "certainty").detach().to(torch.float32).reshape(B, -1).contiguous()
        if certainty.shape[1] != n:
            raise ValueError(f"roma_amd.triangulation: certainty has {certainty.shape[1]} entries per pair for {n} matches")
    f32 = dict(device=dev, dtype=torch.float32)
    points = torch.empty((B, n, 3), **f32)
    depth_other, reproj, parallax = (torch.empty((B, n), **f32) for _ in range(3))
    flags = torch.empty((B, n), device=dev, dtype=torch.uint8)
    stats = torch.zeros((B, 2, 8), device=dev, dtype=torch.int32)
    if B > 0 and n > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_triangulate(
                _ptr(m), _ptr(certainty), _ptr(counts), _ptr(valid), _ptr(R), _ptr(t), _ptr(K_A), _ptr(K_B), B, n, int(coords), *sizes,
                int(sym_w), *thresholds, _ptr(points), _ptr(depth_other), _ptr(reproj), _ptr(parallax), _ptr(flags), _ptr(stats),
                _stream(dev)))
    return Triangulation(points, depth_other, reproj, parallax, flags, flags == 0, stats), (R, t, K_A, K_B)


def triangulate(kpts_A, kpts_B, R, t, K_A=None, K_B=None, certainty=None, counts=None, valid=None, max_depth=math.inf,
                max_reproj=math.inf, min_parallax=0.0, min_certainty=0.0):
    """Depth and 3-D point of every match under the pose (R, t), on the device with no host synchronisation
    (`roma_op_triangulate`).  kpts_A, kpts_B [B, N, 2] pixel coordinates (as `estimate_pose` takes them), or kpts_A one
    [B, N, 4] tensor (columns 0:2 in A, 2:4 in B; float32 contiguous is read in place) with kpts_B None.  Image A is the
    reference: its pixel is taken as exact, the point lies on its ray.  R [B, 3, 3], t [B, 3] or [B, 3, 1] float64 (A to B);
    K_A, K_B [3, 3] or [B, 3, 3], numpy or tensor, None for identity (normalised points); certainty [B, N]; counts [B] rows per
    pair; valid [B] bool, pairs to triangulate (e.g. `estimate_pose`'s ok).

    Returns Triangulation(points [B, N, 3] float32 in camera A's frame - points[..., 2] is the depth -, depth_other [B, N] (the
    depth in camera B), reproj [B, N] (signed distance of the B keypoint from the epipolar line, pixels of B), parallax [B, N]
    (degrees), flags [B, N] uint8, valid [B, N] bool = flags == 0, stats [B, 2, 8] int32).  Flag bits: 1 skipped (beyond counts,
    or the pair is not valid), 2 degenerate (non-finite input, the pixel at the epipole, t = 0), 4 cheirality (not 0 < depth <
    max_depth in both cameras), 8 |reproj| > max_reproj, 16 parallax < min_parallax, 32 certainty < min_certainty; rows with bit
    1 or 2 hold NaN.  stats[:, 0] = (rows considered, valid, degenerate, cheirality, reproj, parallax, certainty, 0).
    The single-pair forms ([N, 2] or [N, 4] keypoints) return everything without the batch axis."""
    if kpts_B is None:
        m = _device_tensor(kpts_A, "matches")
        if m.dim() not in (2, 3) or m.shape[-1] != 4:
            raise ValueError(f"roma_amd.triangulation: without kpts_B the matches must be [N, 4] or [B, N, 4], got {tuple(m.shape)}")
        single = m.dim() == 2
        m = m.detach().to(torch.float32).contiguous()
        m = m[None] if single else m
    else:
        single = isinstance(kpts_A, torch.Tensor) and kpts_A.dim() == 2
        a, b = _pair_batch(kpts_A, kpts_B)
        m = torch.cat((a, b), dim=-1)
    out, _ = _launch(m, certainty, R, t, K_A, K_B, counts, valid, 0, (0, 0, 0, 0), 0,
                     _thresholds(max_depth, max_reproj, min_parallax, min_certainty))
    return Triangulation(*(o[0] for o in out)) if single else out


def _view_poses(K, R, t, view_valid, B, V, dev):
    """the per-view arguments of `triangulate_views` as [B, V, ..] device tensors (K and view_valid may be None)"""
    from .bundle import _view_cameras
    R, t = _device_tensor(R, "R"), _device_tensor(t, "t")
    if R.numel() != B * V * 9 or t.numel() != B * V * 3:
        raise ValueError(f"roma_amd.triangulation: R and t must hold {B} x {V} poses, got {tuple(R.shape)} and {tuple(t.shape)}")
    R = R.detach().to(device=dev, dtype=torch.float64).reshape(B, V, 3, 3).contiguous()
    t = t.detach().to(device=dev, dtype=torch.float64).reshape(B, V, 3).contiguous()
    if view_valid is not None:
        view_valid = torch.as_tensor(view_valid).to(device=dev)
        view_valid = view_valid[None].expand(B, V) if tuple(view_valid.shape) == (V,) else view_valid
        if tuple(view_valid.shape) != (B, V):
            raise ValueError(f"roma_amd.triangulation: view_valid must be [{V}] or [{B}, {V}], got {tuple(view_valid.shape)}")
        view_valid = (view_valid != 0).to(torch.uint8).contiguous()
    return _view_cameras(K, B, V, dev), R, t, view_valid


def triangulate_views(kpts, K, R, t, view_valid=None, counts=None, valid=None, max_reproj=math.inf, min_parallax=0.0,
                      max_depth=math.inf, min_views=2, gn_steps=3, trim=True):
    """The 3-D point of every track from all the views that observe it, the poses given (`roma_op_triangulate_views`): the point
    half of `bundle_adjust`, on the device with no host synchronisation.  kpts [B, V, N, 2] pixels of V <= 8 views (read as
    float32; a non-finite entry: the view does not observe the point - what `build_tracks` writes), K [V, 3, 3], [3, 3] or
    [B, V, 3, 3] (None: kpts are normalised image coordinates, and so is max_reproj), R [B, V, 3, 3], t [B, V, 3] with
    x_cam = R X + t; view_valid [B, V] bool: a view that is not valid contributes no observation (an unregistered view);
    counts [B] points per problem, valid [B] bool problems to triangulate.  [V, N, 2] with [V, ..] poses is one problem.

    Per point, in float64 (restated by tools/triangulate_views_ref.py): the midpoint of the rays of the observations in use, up
    to gn_steps (<= 10) Gauss-Newton steps on the reprojection error, each kept only if it lowers the cost; with trim, while
    the largest error exceeds max_reproj (pixels of its view, divided by (fx + fy) / 2 as in `bundle_adjust`) and at least
    three observations are in use, the worst one leaves and the point is computed again.

    Returns ViewsTriangulation(points [B, N, 3] float64, reproj [B, V, N] float32 (pixels; every observation of a valid view,
    trimmed ones included; NaN elsewhere), used [B, V, N] bool (the observations of the final fit), parallax [B, N] float32
    (largest angle between two rays in use, degrees), flags [B, N] uint8, valid [B, N] bool = flags == 0, stats [B, 8] int32 =
    (points considered, valid, degenerate, cheirality, reproj, parallax, observations trimmed, 0)).  Flag bits as for
    `triangulate`: 1 skipped, 2 degenerate (fewer than min_views observations in use, parallel rays), 4 not 0 < depth <
    max_depth in a view in use, 8 an observation in use above max_reproj, 16 parallax < min_parallax; points with bit 1 or 2
    are NaN, so the array feeds `bundle_adjust` unchanged."""
    th = tuple(float(x) for x in (max_reproj, min_parallax, max_depth))
    if not all(x >= 0 for x in th):
        raise ValueError("roma_amd.triangulation: max_reproj, min_parallax and max_depth must not be negative")
    if not 0 <= int(gn_steps) <= MAX_GN:
        raise ValueError(f"roma_amd.triangulation: need 0 <= gn_steps <= {MAX_GN}")
    if not isinstance(kpts, torch.Tensor) or kpts.dim() not in (3, 4) or kpts.shape[-1] != 2:
        raise ValueError("roma_amd.triangulation: kpts must be a tensor [V, N, 2] or [B, V, N, 2]")
    single = kpts.dim() == 3
    B, V, N = (1 if single else int(kpts.shape[0])), int(kpts.shape[-3]), int(kpts.shape[-2])
    if not 2 <= V <= MAX_VIEWS or not 2 <= int(min_views) <= V:
        raise ValueError(f"roma_amd.triangulation: need 2 <= V <= {MAX_VIEWS} views and 2 <= min_views <= V, got V = {V}")
    if B * V * N >= 2 ** 31 or B > 65535:
        raise ValueError(f"roma_amd.triangulation: {B} x {V} x {N} observations is more than one call takes")
    x = _device_tensor(kpts, "kpts")
    dev = x.device
    x = x.detach().to(torch.float32).contiguous().reshape(B, V, N, 2)
    K, R, t, view_valid = _view_poses(K, R, t, view_valid, B, V, dev)
    counts, valid = _counts(counts, B, dev), _valid(valid, B, dev)
    points = torch.full((B, N, 3), float("nan"), device=dev, dtype=torch.float64)
    reproj = torch.full((B, V, N), float("nan"), device=dev, dtype=torch.float32)
    used = torch.zeros((B, V, N), device=dev, dtype=torch.bool)
    parallax = torch.full((B, N), float("nan"), device=dev, dtype=torch.float32)
    flags = torch.full((B, N), SKIPPED, device=dev, dtype=torch.uint8)
    stats = torch.zeros((B, 8), device=dev, dtype=torch.int32)
    if B > 0 and N > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_triangulate_views(
                _ptr(x), _ptr(K), _ptr(R), _ptr(t), _ptr(view_valid), _ptr(counts), _ptr(valid), B, V, N, *th, int(min_views),
                int(gn_steps), int(bool(trim)), _ptr(points), _ptr(reproj), _ptr(used), _ptr(parallax), _ptr(flags), _ptr(stats),
                _stream(dev)))
    out = ViewsTriangulation(points, reproj, used, parallax, flags, flags == 0, stats)
    return ViewsTriangulation(*(o[0] for o in out)) if single else out


def _consistency(points, flags, R, t, K_A, K_B, sizes, H, W, rel_thresh, want_err):
    B, dev = int(points.shape[0]), points.device
    if not (float(rel_thresh) >= 0):
        raise ValueError("roma_amd.triangulation: rel_thresh must not be negative")
    consistent = torch.empty((B, H, 2 * W), device=dev, dtype=torch.uint8)
    err = torch.empty((B, H, 2 * W), device=dev, dtype=torch.float32) if want_err else None
    if B > 0 and H > 0 and W > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_depth_consistency(_ptr(points), _ptr(flags), _ptr(R), _ptr(t), _ptr(K_A), _ptr(K_B), *sizes,
                                                             B, H, W, float(rel_thresh), _ptr(consistent), _ptr(err), _stream(dev)))
    return consistent, err


def depth_consistency(points, flags, R, t, K_A, K_B, H_A, W_A, H_B=None, W_B=None, rel_thresh=0.05, return_err=False):
    """The mutual check of the two halves of a symmetric triangulation (`roma_op_depth_consistency`): points [B, H, 2W, 3] and
    flags [B, H, 2W] of `triangulate_warp(..., symmetric=True)` (or of one pair, without B).  Every valid point is moved to the
    other camera's frame, projected, and its depth there compared with the other half's own depth, interpolated bilinearly
    (align_corners=False) from four valid neighbours.  Returns consistent uint8 [B, H, 2W]: 1 the relative difference is below
    rel_thresh, 0 it is not, 2 no support (the projection leaves the grid, a neighbour is not valid) or the point itself is not
    valid; with return_err also err float32 [B, H, 2W], NaN where there is no support."""
    points, flags = _device_tensor(points, "points"), _device_tensor(flags, "flags")
    single = points.dim() == 3
    if points.dim() not in (3, 4) or points.shape[-1] != 3 or points.shape[-2] % 2 or tuple(points.shape[:-1]) != tuple(flags.shape):
        raise ValueError(f"roma_amd.triangulation: expected points [B, H, 2W, 3] and flags [B, H, 2W], got {tuple(points.shape)} and "
                         f"{tuple(flags.shape)}")
    H, W = int(points.shape[-3]), int(points.shape[-2]) // 2
    p = points.detach().to(torch.float32).reshape(-1, H, 2 * W, 3).contiguous()
    f = flags.detach().to(torch.uint8).reshape(-1, H, 2 * W).contiguous()
    B, dev = int(p.shape[0]), p.device
    R, t = _pose_tensor(R, "R", B, (3, 3), dev), _pose_tensor(t, "t", B, (3, 1), dev).reshape(B, 3)
    sizes = _sizes(H_A, W_A, H_B, W_B)
    out = _consistency(p, f, R, t, _cameras(K_A, B, dev), _cameras(K_B, B, dev), sizes, H, W, rel_thresh, return_err)
    out = tuple(o[0] for o in out if o is not None) if single else tuple(o for o in out if o is not None)
    return out if return_err else out[0]


def _sizes(H_A, W_A, H_B, W_B):
    sizes = (int(W_A), int(H_A), int(W_A if W_B is None else W_B), int(H_A if H_B is None else H_B))
    if min(sizes) <= 0:
        raise ValueError("roma_amd.triangulation: image sizes must be positive")
    return sizes


def triangulate_warp(warp, certainty, R, t, K_A, K_B, H_A, W_A, H_B=None, W_B=None, symmetric=None, consistency=False,
                     rel_thresh=0.05, counts=None, valid=None, max_depth=math.inf, max_reproj=math.inf, min_parallax=0.0,
                     min_certainty=0.0):
    """Depth maps and point clouds of a dense warp, on the device with no host synchronisation: `match()` output
    warp [B, H, W, 4] (or [B, H, 2W, 4] from a symmetric matcher) in normalised [-1, 1] coordinates, read in place, and certainty
    (or None) with the pose R [B, 3, 3], t [B, 3] / [B, 3, 1] from A to B, the cameras K_A, K_B and the image sizes the cameras
    refer to (H_B, W_B default to those of A).  symmetric: whether the right half of the grid is image B's own grid; None takes
    it from the shape (an even width of at least twice the height) - `RegressionMatcher.triangulate_warp` passes the matcher's.
    valid [B] bool: pairs to triangulate (e.g. `estimate_pose`'s ok); thresholds as for `triangulate`.

    Returns a WarpTriangulation (a dict with attribute access): depth_A [B, H, W], points_A [B, H, W, 3] (camera A's frame),
    valid_A [B, H, W] bool, reproj_A, parallax_A, flags_A and stats [B, 2, 8]; for a symmetric warp also the _B set from the right
    half (image B's grid, points in camera B's frame) and, with consistency=True, consistent_A and consistent_B (uint8: 1
    consistent, 0 not, 2 no support; see `depth_consistency`).  The entries are views of [B, H, 2W] outputs.  A single pair
    ([H, W, 4]) returns everything without the batch axis."""
    warp = _device_tensor(warp, "warp")
    if warp.dim() not in (3, 4) or warp.shape[-1] != 4:
        raise ValueError(f"roma_amd.triangulation: warp must be [B, H, W, 4] or [H, W, 4], got {tuple(warp.shape)}")
    single = warp.dim() == 3
    H, Wd = int(warp.shape[-3]), int(warp.shape[-2])
    if symmetric is None:
        symmetric = Wd % 2 == 0 and Wd >= 2 * H
    if symmetric and Wd % 2:
        raise ValueError(f"roma_amd.triangulation: a symmetric warp has an even width, got {Wd}")
    if consistency and not symmetric:
        raise ValueError("roma_amd.triangulation: consistency needs a symmetric warp")
    W = Wd // 2 if symmetric else Wd
    w32 = warp.detach().to(torch.float32).contiguous()
    B = 1 if single else int(w32.shape[0])
    sizes = _sizes(H_A, W_A, H_B, W_B)
    tri, (R, t, K_A, K_B) = _launch(w32.reshape(B, H * Wd, 4), certainty, R, t, K_A, K_B, counts, valid, 1, sizes,
                                    W if symmetric else 0, _thresholds(max_depth, max_reproj, min_parallax, min_certainty))
    grid = {"points": tri.points.reshape(B, H, Wd, 3), "reproj": tri.reproj.reshape(B, H, Wd),
            "parallax": tri.parallax.reshape(B, H, Wd), "flags": tri.flags.reshape(B, H, Wd), "valid": tri.valid.reshape(B, H, Wd)}
    grid["depth"] = grid["points"][..., 2]
    if consistency:
        grid["consistent"] = _consistency(tri.points, tri.flags, R, t, K_A, K_B, sizes, H, W, rel_thresh, False)[0]
    out = WarpTriangulation(stats=tri.stats[0] if single else tri.stats)
    for half, name in enumerate("AB" if symmetric else "A"):
        for key, val in grid.items():
            v = val[:, :, half * W:(half + 1) * W]
            out[f"{key}_{name}"] = v[0] if single else v
    return out
