"""Point-cloud rendering on the device (`roma_op_render_points`, csrc/point_render.hip): what a dense reconstruction is looked at,
localised against and checked with.  The N rows of a world-space cloud - `DenseFusion.points` as it is, NaN padding included - are
splatted into C cameras with a z-buffer of packed 64-bit keys (nearest depth, then lowest row), back-surface points that show
through the gaps of a nearer surface are removed, small holes are closed, and depth, row index, colour and a mask come out per
pixel of every frame.  The steps are spelled out in include/roma_hip.h and restated in numpy float64 by tools/point_render_ref.py;
the result is bit-identical from run to run and independent of the batch and of the other frames.  Device tensors only, one
enqueue for a batch of problems, nothing read back.  Known: at a depth edge the nearer surface grows by up to occlusion_radius +
fill_radius pixels."""
from __future__ import annotations

import math
from functools import partial
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream
from .geometry import _valid

MAX_RADIUS = 4                      # csrc/point_render.hip: RENDER_MAX_RADIUS
HIT, REMOVED, FILLED = 1, 2, 4      # bits of `mask`


class PointRender(NamedTuple):
    color: Optional[torch.Tensor]  # [.., C, H, W, 3] uint8 (None without colors): the row's colour, background where there is none
    depth: torch.Tensor            # [.., C, H, W] float32: the depth in the camera, NaN where there is none
    index: torch.Tensor            # [.., C, H, W] int32: the row of the cloud, -1 where there is none
    mask: torch.Tensor             # [.., C, H, W] uint8: bit 0 hit by the splat, bit 1 removed by the occlusion filter, bit 2 filled
    stats: torch.Tensor            # [.., C, 4] int32: usable rows whose cell lies inside the image, pixels hit, removed, filled


_device_tensor = partial(_lib._device_tensor, module="point_render")


def orbit_cameras(R0, t0, centre, angles, axis=(0.0, 1.0, 0.0), device="cuda"):
    """The turntable: the camera (R0, t0), x_cam = R0 X + t0, rotated about the world point `centre` by each of `angles` (radians)
    about `axis` (a world direction, normalised here).  With Q the rotation by the angle, the camera is moved by X -> Q (X - centre)
    + centre: R = R0 Q^T, t = R0 (centre - Q^T centre) + t0, so `centre` keeps its place in the camera frame and angle 0 returns
    (R0, t0) bit for bit.  Built in float64 on the host from host values; returns (R [C, 3, 3], t [C, 3]) float64 on `device`."""
    R0 = np.asarray(R0.detach().cpu() if isinstance(R0, torch.Tensor) else R0, dtype=np.float64)
    t0 = np.asarray(t0.detach().cpu() if isinstance(t0, torch.Tensor) else t0, dtype=np.float64).reshape(-1)
    c = np.asarray(centre.detach().cpu() if isinstance(centre, torch.Tensor) else centre, dtype=np.float64).reshape(-1)
    k = np.asarray(axis, dtype=np.float64).reshape(-1)
    angles = np.asarray(angles.detach().cpu() if isinstance(angles, torch.Tensor) else angles, dtype=np.float64).reshape(-1)
    if R0.shape != (3, 3) or t0.shape != (3,) or c.shape != (3,) or k.shape != (3,):
        raise ValueError("roma_amd.point_render: orbit_cameras takes R0 [3, 3], t0 [3], centre [3] and axis [3]")
    if len(angles) < 1 or not np.isfinite(angles).all():
        raise ValueError("roma_amd.point_render: orbit_cameras needs at least one finite angle")
    norm = float(np.linalg.norm(k))
    if not (np.isfinite(norm) and norm > 0):
        raise ValueError("roma_amd.point_render: the axis must not be zero")
    k = k / norm
    cross = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R, t = np.empty((len(angles), 3, 3)), np.empty((len(angles), 3))
    for i, a in enumerate(angles):
        if a == 0.0:
            R[i], t[i] = R0, t0
            continue
        Q = math.cos(a) * np.eye(3) + math.sin(a) * cross + (1.0 - math.cos(a)) * np.outer(k, k)  # Rodrigues
        R[i] = R0 @ Q.T
        t[i] = R0 @ (c - Q.T @ c) + t0
    return torch.as_tensor(R, device=device), torch.as_tensor(t, device=device)


def _shapes(points, K, R, t, colors, counts):
    """(B, N, C, single) after every shape check: nothing here asks for a device"""
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise ValueError("roma_amd.point_render: points must be a tensor [N, 3] or [B, N, 3]")
    single = points.dim() == 2
    B, N = (1 if single else int(points.shape[0])), int(points.shape[-2])
    if not isinstance(R, torch.Tensor) or not isinstance(t, torch.Tensor) or R.dim() not in (3, 4) or tuple(R.shape[-2:]) != (3, 3):
        raise ValueError("roma_amd.point_render: R must be a tensor [C, 3, 3] or [B, C, 3, 3] and t a tensor")
    C = int(R.shape[-3])
    if C < 1:
        raise ValueError("roma_amd.point_render: need at least one camera")
    if R.dim() == 4 and (single or int(R.shape[0]) != B):
        raise ValueError(f"roma_amd.point_render: R {tuple(R.shape)} does not match {B} problem(s)" + (" without a batch axis" if single else ""))
    if tuple(t.shape) != tuple(R.shape[:-2]) + (3,):
        raise ValueError(f"roma_amd.point_render: t must be {list(R.shape[:-2]) + [3]}, got {tuple(t.shape)}")
    if B * C > 65535:
        raise ValueError("roma_amd.point_render: at most 65535 frames per call (B * C)")
    if K is None or tuple(np.shape(K)) not in ((3, 3), (C, 3, 3), (B, C, 3, 3)):
        raise ValueError(f"roma_amd.point_render: K must be [3, 3], [{C}, 3, 3] or [{B}, {C}, 3, 3] (the cameras in output pixels)")
    if colors is not None and (not isinstance(colors, torch.Tensor) or tuple(colors.shape) != tuple(points.shape) or colors.dtype != torch.uint8):
        raise ValueError(f"roma_amd.point_render: colors must be a uint8 tensor {list(points.shape)} or None")
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.numel() != B or counts.dtype.is_floating_point):
        raise ValueError(f"roma_amd.point_render: counts must be an integer tensor with {B} entries or None")
    return B, N, C, single


def render_points(points, K, R, t, H, W, *, colors=None, counts=None, radius=1, near=1e-6, far=math.inf, occlusion_radius=2,
                  occlusion_rel=0.05, occlusion_count=3, fill_radius=1, fill_min=3, background=(0, 0, 0), valid=None):
    """A point cloud rendered into C cameras: depth, row index, colour and a mask per pixel (`roma_op_render_points`).

    points [B, N, 3] float32 world points ([N, 3] is one problem); rows with a coordinate that is not finite - the padding of
    `DenseFusion.points` - are skipped, as are rows at and beyond counts [B].  colors [B, N, 3] uint8 or None.  K [3, 3], [C, 3, 3] or
    [B, C, 3, 3]: the cameras IN UNITS OF THE OUTPUT PIXEL, the centre of pixel (r, c) at (c + 0.5, r + 0.5) - the convention of
    `fuse_depth_maps`, so a view's own grid camera renders onto its own grid.  R [B, C, 3, 3] or [C, 3, 3], t [B, C, 3] or [C, 3] with
    x_cam = R X + t; poses without the batch axis serve every problem.  valid [B]: a problem that is not valid renders empty.

      1. a row with near <= depth <= far whose cell (floor(v), floor(u)) lies within `radius` of the image offers its depth and
         its row to the (2 radius + 1)^2 pixels around the cell; a pixel keeps the nearest depth, then the lowest row
      2. occlusion_radius o > 0: a hit pixel is removed when at least occlusion_count hit pixels of its (2 o + 1)^2 window are
         nearer by more than occlusion_rel (z > z_q (1 + occlusion_rel)) - a back surface showing through the gaps of a nearer one
      3. fill_radius f > 0: an empty or removed pixel with at least fill_min surviving pixels in its (2 f + 1)^2 window takes the
         nearest of them
    At a depth edge the nearer surface grows by up to o + f pixels.  `radius=0, occlusion_radius=0, fill_radius=0` is the plain
    z-buffer.  All three radii lie in [0, 4].

    Returns PointRender(color, depth, index, mask, stats); the single-problem form returns everything without the batch axis.
    No host synchronisation."""
    B, N, C, single = _shapes(points, K, R, t, colors, counts)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or 3 * B * C * H * W >= 2 ** 31:
        raise ValueError(f"roma_amd.point_render: the frame must not be empty and 3 B C H W must stay below 2^31, got {H} x {W}")
    radius, o_rad, f_rad = int(radius), int(occlusion_radius), int(fill_radius)
    if not (0 <= radius <= MAX_RADIUS and 0 <= o_rad <= MAX_RADIUS and 0 <= f_rad <= MAX_RADIUS):
        raise ValueError(f"roma_amd.point_render: radius, occlusion_radius and fill_radius must lie in [0, {MAX_RADIUS}]")
    o_cnt, f_min = int(occlusion_count), int(fill_min)
    if o_cnt < 1 or f_min < 1:
        raise ValueError("roma_amd.point_render: occlusion_count and fill_min must be at least 1")
    near, far, o_rel = float(near), float(far), float(occlusion_rel)
    if not o_rel >= 0 or not near > 0 or not far >= near:
        raise ValueError("roma_amd.point_render: need occlusion_rel >= 0, near > 0 and far >= near")
    bg = [int(x) for x in background]
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise ValueError("roma_amd.point_render: background is three values in [0, 255]")
    points = _device_tensor(points, "points").to(torch.float32).reshape(B, N, 3).contiguous()
    dev = points.device
    if colors is not None:
        colors = _device_tensor(colors, "colors").to(device=dev).reshape(B, N, 3).contiguous()
    if counts is not None:
        counts = _device_tensor(counts, "counts").to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    R = _device_tensor(R, "R").to(device=dev, dtype=torch.float64)
    t = _device_tensor(t, "t").to(device=dev, dtype=torch.float64)
    if R.dim() == 3:
        R, t = R[None].expand(B, C, 3, 3), t[None].expand(B, C, 3)
    R, t = R.contiguous(), t.contiguous()
    from .bundle import _view_cameras
    K = _view_cameras(K, B, C, dev)
    valid = _valid(valid, B, dev)
    color = torch.empty((B, C, H, W, 3), device=dev, dtype=torch.uint8) if colors is not None else None
    depth = torch.empty((B, C, H, W), device=dev, dtype=torch.float32)
    index = torch.empty((B, C, H, W), device=dev, dtype=torch.int32)
    mask = torch.empty((B, C, H, W), device=dev, dtype=torch.uint8)
    stats = torch.zeros((B, C, 4), device=dev, dtype=torch.int32)
    if B > 0:
        if N == 0:  # an empty tensor has no address, and the entry refuses a null pointer: N = 0 renders empty from one unread row
            points = torch.zeros((B, 1, 3), device=dev, dtype=torch.float32)
            colors = None if colors is None else torch.zeros((B, 1, 3), device=dev, dtype=torch.uint8)
        lib = _lib.load()
        nws = int(lib.roma_op_render_points_workspace(B, C, H, W))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_render_points(
                _ptr(points), _ptr(colors), _ptr(counts), _ptr(valid), _ptr(K), _ptr(R), _ptr(t), B, N, C, H, W, radius, near, far, o_rad,
                o_rel, o_cnt, f_rad, f_min, bg[0] | bg[1] << 8 | bg[2] << 16, _ptr(color), _ptr(depth), _ptr(index), _ptr(mask),
                _ptr(stats), _ptr(ws), nws, _stream(dev)))
    out = PointRender(color, depth, index, mask, stats)
    return PointRender(*(None if o is None else o[0] for o in out)) if single else out
