"""Dense multi-view depth fusion on the device (`roma_op_fuse_depth_maps`, `roma_op_relative_poses`, csrc/depth_fusion.hip): what
joins the poses of an image set to a dense reconstruction.  With the P pairs of V <= 8 views triangulated by one
`triangulate_warp` call, every view owns up to 14 depth hypotheses per pixel; a vote selects among them, the fused depth maps
check one another across views (seen / violated / occluded), a surface point several views keep is emitted once, and what stays
is numbered into one point cloud in (view, pixel) order.  The steps are spelled out in include/roma_hip.h and restated in numpy
float64 by tools/depth_fusion_ref.py; the result is bit-identical from run to run and independent of the batch.  Device tensors
only, one enqueue for a batch of problems, nothing read back."""
from __future__ import annotations

from functools import partial
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream
from .geometry import _valid

MAX_VIEWS, MAX_PAIRS = 8, 64          # csrc/depth_fusion.hip: FUSE_MAX_VIEWS, FUSE_MAX_PAIRS
MAX_SLOTS = 2 * (MAX_VIEWS - 1)       # FUSE_MAX_SLOTS
MAX_COLOR_VIEWS = 128                 # FUSE_MAX_COLOR_VIEWS: B * V with a colour source
KEPT, DUPLICATE = 1, 2                # bits of `state`


class DenseFusion(NamedTuple):
    depth: torch.Tensor         # [.., V, H, W] float32: the fused depth of every view, NaN where there is none
    weight: torch.Tensor        # [.., V, H, W] float32: the summed weight of the winner's supporters, 0 where there is no depth
    support: torch.Tensor       # [.., V, H, W] uint8: the supporters of the winner (the best count where it is below min_support)
    seen: torch.Tensor          # [.., V, H, W] uint8: bit u - view u sees the point at the same depth
    violated: torch.Tensor      # [.., V, H, W] uint8: bit u - the point floats in front of the surface view u sees
    state: torch.Tensor         # [.., V, H, W] uint8: bit 0 kept, bit 1 duplicate of a kept pixel of a lower view
    points: torch.Tensor        # [.., max_points, 3] float32 world points in (view, row-major pixel) order, NaN padding
    colors: Optional[torch.Tensor]  # [.., max_points, 3] uint8 (None without images), 0 padding
    cloud_weight: torch.Tensor  # [.., max_points] float32, 0 padding
    source: torch.Tensor        # [.., max_points, 2] int32: (view, pixel index r W + c), -1 padding
    counts: torch.Tensor        # [..] int32 = min(total, max_points)
    total: torch.Tensor         # [..] int32: the points there are
    stats: torch.Tensor         # [.., 8] int32: pixels with a hypothesis, fused, kept, duplicates, emitted, with a violation, 0, 0


_device_tensor = partial(_lib._device_tensor, module="depth_fusion")


def _pairs(pair_views, V, unique):
    if isinstance(pair_views, torch.Tensor) and pair_views.is_cuda:
        raise ValueError("roma_amd.depth_fusion: pair_views is host data (a list of tuples): it is checked before anything is launched")
    pv = np.ascontiguousarray(np.asarray(pair_views, dtype=np.int32).reshape(-1, 2))
    if not 1 <= len(pv) <= MAX_PAIRS:
        raise ValueError(f"roma_amd.depth_fusion: need 1 .. {MAX_PAIRS} pairs, got {len(pv)}")
    if pv.min() < 0 or pv.max() >= V or (pv[:, 0] == pv[:, 1]).any():
        raise ValueError(f"roma_amd.depth_fusion: pair_views must hold two different views in [0, {V}) per row")
    if unique and len({(int(a), int(b)) for a, b in pv}) != len(pv):
        raise ValueError("roma_amd.depth_fusion: pair_views holds an ordered pair twice ((i, j) and (j, i) may both occur)")
    return pv


def _pose_shapes(R, t):
    """(B, V, single) of R [V, 3, 3] or [B, V, 3, 3] and t, checked before any device is asked for"""
    if not isinstance(R, torch.Tensor) or not isinstance(t, torch.Tensor) or R.dim() not in (3, 4) or tuple(R.shape[-2:]) != (3, 3):
        raise ValueError("roma_amd.depth_fusion: R must be a tensor [V, 3, 3] or [B, V, 3, 3] and t a tensor")
    single = R.dim() == 3
    B, V = (1 if single else int(R.shape[0])), int(R.shape[-3])
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError(f"roma_amd.depth_fusion: need 2 <= V <= {MAX_VIEWS} views, got {V}")
    if B > 65535:
        raise ValueError("roma_amd.depth_fusion: at most 65535 problems per call")
    if t.numel() != B * V * 3:
        raise ValueError(f"roma_amd.depth_fusion: t must hold {B} x {V} translations, got {tuple(t.shape)}")
    return B, V, single


def _poses(R, t, B, V):
    """([B, V, 3, 3], [B, V, 3]) float64 contiguous device tensors"""
    R, t = _device_tensor(R, "R"), _device_tensor(t, "t")
    R = R.detach().to(torch.float64).reshape(B, V, 3, 3).contiguous()
    return R, t.detach().to(device=R.device, dtype=torch.float64).reshape(B, V, 3).contiguous()


def relative_poses(R, t, pair_views):
    """The pose of every pair from the poses of the views (`roma_op_relative_poses`): R [B, V, 3, 3], t [B, V, 3] float64 with
    x_cam = R X + t (or one problem without B), pair_views P tuples (i, j) on the host.  Returns (R_ij [B, P, 3, 3], t_ij
    [B, P, 3]) float64 with R_ij = R_j R_i^T and t_ij = t_j - R_ij t_i, the (A to B) pose `triangulate_warp` takes for pair
    (i, j).  One tiny launch, no host synchronisation."""
    B, V, single = _pose_shapes(R, t)
    pv = _pairs(pair_views, V, False)
    P = len(pv)
    R, t = _poses(R, t, B, V)
    dev = R.device
    Rij = torch.empty((B, P, 3, 3), device=dev, dtype=torch.float64)
    tij = torch.empty((B, P, 3), device=dev, dtype=torch.float64)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_relative_poses(_ptr(R), _ptr(t), pv.ctypes.data, B, V, P, _ptr(Rij), _ptr(tij), _stream(dev)))
    return (Rij[0], tij[0]) if single else (Rij, tij)


def _colour_source(images, B, V, single, dev):
    """(packed uint8 device tensor, offsets int64 [B, V], sizes int32 [B, V, 2]) of B x V uint8 device images [H_img, W_img, 3]"""
    rows = [images] if single else images
    if not isinstance(rows, (list, tuple)) or len(rows) != B or any(not isinstance(r, (list, tuple)) or len(r) != V for r in rows):
        raise ValueError(f"roma_amd.depth_fusion: images must be {V} images per problem" + ("" if single else f", for {B} problems"))
    if B * V > MAX_COLOR_VIEWS:
        raise ValueError(f"roma_amd.depth_fusion: with images B * V must not exceed {MAX_COLOR_VIEWS}")
    flat, offsets, sizes, at = [], [], [], 0
    for row in rows:
        for im in row:
            im = _device_tensor(im, "an image")
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1 or im.device != dev:
                raise ValueError("roma_amd.depth_fusion: every image must be a uint8 tensor [H, W, 3] on the device of points")
            flat.append(im.detach().reshape(-1))
            offsets.append(at)
            sizes.append((int(im.shape[0]), int(im.shape[1])))
            at += int(im.numel())
    return torch.cat(flat), np.asarray(offsets, dtype=np.int64).reshape(B, V), np.asarray(sizes, dtype=np.int32).reshape(B, V, 2)


def fuse_depth_maps(points, flags, certainty, pair_views, K, R, t, *, symmetric=None, images=None, rel_thresh=0.01, min_support=2,
                    min_consistent=1, max_violations=0, dedupe=True, max_points=None, view_valid=None, valid=None):
    """The depth maps of the pairs of an image set to one depth map per view and one point cloud (`roma_op_fuse_depth_maps`).

    points [B, P, H, Wd, 3] float32, flags [B, P, H, Wd] uint8 and certainty [B, P, H, Wd] float32 (or None: every weight 1) are
    the outputs of ONE `triangulate_warp` call over the P pairs of each problem, read in place (the depth is points[..., 2]);
    [P, H, Wd, 3] is one problem.  pair_views: P tuples (i, j) on the host, i != j, no ordered pair twice; with symmetric (Wd =
    2W) the left half lies on the grid of view i and the right half on the grid of view j, without it only the first.  K
    [V, 3, 3], [3, 3] or [B, V, 3, 3]: the cameras IN GRID UNITS (image intrinsics scaled by W / W_img and H / H_img; the centre of
    cell (r, c) is (c + 0.5, r + 0.5)); R [B, V, 3, 3], t [B, V, 3] with x_cam = R X + t; view_valid [B, V] or [V], valid [B].
    images: V uint8 device tensors [H_img, W_img, 3] (per problem: a list of B such lists) - the colour of a point is the image
    pixel that holds the centre of its cell.

    Per pixel of a view: the hypotheses whose flag byte is 0 with a finite positive depth and weight vote - l supports k when
    |z_l - z_k| <= rel_thresh min(z_l, z_k); the winner has the most supporters, then the largest summed weight, then the lowest
    slot, and with at least min_support of them the depth is their weighted mean.  A fused pixel is moved into every other valid
    view and compared with that view's fused depth (bilinear from four neighbours that all have one): within rel_thresh it is
    `seen`, in front of it `violated`, behind it occluded.  It is kept with at least min_consistent bits in seen and at most
    max_violations in violated; with dedupe a kept pixel is a duplicate when a lower view that sees it keeps the pixel nearest
    its projection.  Kept pixels that are no duplicates are the cloud, in (view, row-major pixel) order, cut at max_points
    (default V H W).

    Returns DenseFusion; the single-problem form returns everything without the batch axis.  No host synchronisation."""
    B, V, single_pose = _pose_shapes(R, t)
    pv = _pairs(pair_views, V, True)
    P = len(pv)
    if not isinstance(points, torch.Tensor) or points.dim() not in (4, 5) or points.shape[-1] != 3:
        raise ValueError("roma_amd.depth_fusion: points must be a tensor [P, H, Wd, 3] or [B, P, H, Wd, 3]")
    single = points.dim() == 4
    if single != single_pose or (1 if single else int(points.shape[0])) != B or int(points.shape[-4]) != P:
        raise ValueError(f"roma_amd.depth_fusion: points {tuple(points.shape)} do not match {B} problem(s) of {P} pairs")
    H, Wd = int(points.shape[-3]), int(points.shape[-2])
    if symmetric is None:
        symmetric = Wd % 2 == 0 and Wd >= 2 * H
    symmetric = bool(symmetric)
    if H < 1 or Wd < 1 or (symmetric and Wd % 2):
        raise ValueError(f"roma_amd.depth_fusion: the grid must not be empty and a symmetric one has an even width, got {H} x {Wd}")
    W = Wd // 2 if symmetric else Wd
    if not isinstance(flags, torch.Tensor) or tuple(flags.shape) != tuple(points.shape[:-1]):
        raise ValueError(f"roma_amd.depth_fusion: flags must be {list(points.shape[:-1])}")
    if certainty is not None and (not isinstance(certainty, torch.Tensor) or tuple(certainty.shape) != tuple(points.shape[:-1])):
        raise ValueError(f"roma_amd.depth_fusion: certainty must be {list(points.shape[:-1])} or None")
    rel = float(rel_thresh)
    if not rel >= 0:
        raise ValueError("roma_amd.depth_fusion: rel_thresh must not be negative")
    min_support, min_consistent, max_violations = int(min_support), int(min_consistent), int(max_violations)
    if not 1 <= min_support <= MAX_SLOTS or not 0 <= min_consistent <= MAX_VIEWS - 1 or max_violations < 0:
        raise ValueError(f"roma_amd.depth_fusion: need 1 <= min_support <= {MAX_SLOTS}, 0 <= min_consistent <= {MAX_VIEWS - 1} and "
                         "max_violations >= 0")
    K_pts = V * H * W if max_points is None else int(max_points)
    if K_pts < 0 or B * P * H * Wd >= 2 ** 31 or B * V * H * W >= 2 ** 31 or 3 * B * K_pts >= 2 ** 31:
        raise ValueError("roma_amd.depth_fusion: more than one call takes (B P H Wd, B V H W and 3 B max_points below 2^31)")
    if K is None:
        raise ValueError("roma_amd.depth_fusion: K is required (the cameras in grid units)")
    R, t = _poses(R, t, B, V)
    dev = R.device
    points = _device_tensor(points, "points").detach().to(torch.float32).contiguous()
    flags = _device_tensor(flags, "flags").detach().to(device=dev, dtype=torch.uint8).contiguous()
    if certainty is not None:
        certainty = _device_tensor(certainty, "certainty").detach().to(device=dev, dtype=torch.float32).contiguous()
    if points.device != dev:
        raise ValueError(f"roma_amd.depth_fusion: points live on {points.device}, the poses on {dev}")
    from .bundle import _view_cameras
    K = _view_cameras(K, B, V, dev)
    if view_valid is not None:
        view_valid = torch.as_tensor(view_valid).to(device=dev)
        view_valid = view_valid[None].expand(B, V) if tuple(view_valid.shape) == (V,) else view_valid
        if tuple(view_valid.shape) != (B, V):
            raise ValueError(f"roma_amd.depth_fusion: view_valid must be [{V}] or [{B}, {V}], got {tuple(view_valid.shape)}")
        view_valid = (view_valid != 0).to(torch.uint8).contiguous()
    valid = _valid(valid, B, dev)
    packed = offsets = sizes = None
    if images is not None:
        packed, offsets, sizes = _colour_source(images, B, V, single, dev)
    f32 = dict(device=dev, dtype=torch.float32)
    u8 = dict(device=dev, dtype=torch.uint8)
    depth, weight = torch.empty((B, V, H, W), **f32), torch.empty((B, V, H, W), **f32)
    support, seen, violated, state = (torch.empty((B, V, H, W), **u8) for _ in range(4))
    out_points = torch.empty((B, K_pts, 3), **f32)
    colors = torch.empty((B, K_pts, 3), **u8) if images is not None else None
    cloud_weight = torch.empty((B, K_pts), **f32)
    source = torch.empty((B, K_pts, 2), device=dev, dtype=torch.int32)
    counts, total = (torch.zeros((B,), device=dev, dtype=torch.int32) for _ in range(2))
    stats = torch.zeros((B, 8), device=dev, dtype=torch.int32)
    if B > 0:
        lib = _lib.load()
        nws = int(lib.roma_op_fuse_depth_maps_workspace(B, V, H, W))
        ws = torch.empty((nws,), **u8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_fuse_depth_maps(
                _ptr(points), _ptr(flags), _ptr(certainty), pv.ctypes.data, _ptr(K), _ptr(R), _ptr(t), _ptr(view_valid), _ptr(valid),
                _ptr(packed), offsets.ctypes.data if offsets is not None else None, sizes.ctypes.data if sizes is not None else None,
                B, V, P, H, W, int(symmetric), rel, min_support, min_consistent, max_violations, int(bool(dedupe)), K_pts,
                _ptr(depth), _ptr(weight), _ptr(support), _ptr(seen), _ptr(violated), _ptr(state), _ptr(out_points), _ptr(colors),
                _ptr(cloud_weight), _ptr(source), _ptr(counts), _ptr(total), _ptr(stats), _ptr(ws), nws, _stream(dev)))
    out = DenseFusion(depth, weight, support, seen, violated, state, out_points, colors, cloud_weight, source, counts, total, stats)
    return DenseFusion(*(None if o is None else o[0] for o in out)) if single else out
