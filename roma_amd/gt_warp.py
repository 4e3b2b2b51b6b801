"""Ground-truth warp from sensor depth and the dense EPE / PCK metrics on the device (`roma_op_warp_kpts`, `roma_op_dense_metrics`,
csrc/gt_warp.hip): the reference's `warp_kpts` and `get_gt_warp` (romatch/utils/utils.py) and
`MegadepthDenseBenchmark.geometric_dist` (romatch/benchmarks/megadepth_dense_benchmark.py) - the consumer of `match()` output that
scores a warp against depth maps, intrinsics and the relative pose.  `dense_metrics` is geometric_dist in one pass: no grid tensor,
no intermediate tensors, no boolean compaction, nothing read back.  The definition is stated in include/roma_hip.h and restated in
numpy float64 by tools/gt_warp_ref.py.

Conventions are those of `roma_amd.triangulation`: device tensors only (the small matrices may also be numpy), T maps camera 0's
frame to camera 1's, no call synchronises with the host.  All arithmetic is float64 in a fixed order, so every output is
bit-identical from run to run and independent of the batch a pair sits in."""
from __future__ import annotations

from collections import namedtuple
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream

DenseMetrics = namedtuple("DenseMetrics", "n_valid n_below gd_sum epe pck prob gd", defaults=(None, None))


def _mode(depth_interpolation_mode, smooth_mask=False):
    if smooth_mask:
        raise NotImplementedError("roma_amd.gt_warp: smooth_mask (the soft consistency mask) is a training-only path and is not implemented")
    if depth_interpolation_mode in ("combined", "nearest-exact"):
        raise NotImplementedError(
            f"roma_amd.gt_warp: depth_interpolation_mode={depth_interpolation_mode!r} is not implemented; the reference passes "
            "'nearest-exact' to F.grid_sample, which torch rejects with a ValueError, so this mode cannot run there either")
    if depth_interpolation_mode != "bilinear":
        raise ValueError(f"roma_amd.gt_warp: depth_interpolation_mode must be 'bilinear', got {depth_interpolation_mode!r}")


def _threshold(x):
    x = float(x)
    if not x >= 0:
        raise ValueError("roma_amd.gt_warp: relative_depth_error_threshold must not be negative")
    return x


def _depth_shape(d, name, B=None):
    if not isinstance(d, torch.Tensor):
        raise TypeError(f"roma_amd.gt_warp: {name} must be a torch tensor, got {type(d).__name__}")
    if d.dim() != 3 or d.dtype != torch.float32 or (B is not None and d.shape[0] != B) or min(d.shape[1:]) < 1:
        want = "[B, H, W]" if B is None else f"[{B}, H, W]"
        raise ValueError(f"roma_amd.gt_warp: {name} must be float32 {want}, got {d.dtype} {tuple(d.shape)}")


def _small_shape(x, name, B, shapes):
    """shape check of T / K given as a tensor or anything numpy takes; returns what `_small` moves to the device"""
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x, dtype=np.float64)
    if tuple(x.shape) not in [(B,) + s for s in shapes]:
        raise ValueError(f"roma_amd.gt_warp: {name} must be " + " or ".join(str([B, *s]) for s in shapes) + f", got {tuple(x.shape)}")
    return x


_device_tensor = partial(_lib._device_tensor, module="gt_warp")


def _small(x, name, dev):
    """T / K as contiguous float64 on the device: a device tensor, or host numpy (uploaded; no synchronisation)"""
    if isinstance(x, torch.Tensor):
        return _device_tensor(x, name).to(device=dev, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C")).to(dev)  # a copy: the caller's array may be read-only


def _pair_shapes(B, depth0, depth1, T, K0, K1, names):
    """shapes and dtypes of what describes the B pairs (B None: taken from depth0); returns (B, T, K0, K1)"""
    _depth_shape(depth0, names[0], B)
    B = int(depth0.shape[0])
    _depth_shape(depth1, names[1], B)
    T = _small_shape(T, names[2], B, ((3, 4), (4, 4)))
    return B, T, _small_shape(K0, names[3], B, ((3, 3),)), _small_shape(K1, names[4], B, ((3, 3),))


def _warp(kpts, grid_hw, depth0, depth1, T, K0, K1, thr, want_valid, want_prob, want_rel, names):
    """roma_op_warp_kpts after every check: (valid bool [B, L] | None, prob f32 [B, L] | None, rel f64 [B, L] | None, warped f64 [B, L, 2])"""
    B = None
    if kpts is not None:
        if not isinstance(kpts, torch.Tensor):
            raise TypeError(f"roma_amd.gt_warp: kpts0 must be a torch tensor, got {type(kpts).__name__}")
        if kpts.dim() != 3 or kpts.shape[-1] != 2 or kpts.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"roma_amd.gt_warp: kpts0 must be float32 or float64 [B, L, 2], got {kpts.dtype} {tuple(kpts.shape)}")
        B = int(kpts.shape[0])
    B, T, K0, K1 = _pair_shapes(B, depth0, depth1, T, K0, K1, names)
    L = int(kpts.shape[1]) if kpts is not None else grid_hw[0] * grid_hw[1]
    if B > 65535 or B * L >= 2 ** 31:
        raise ValueError(f"roma_amd.gt_warp: {B} x {L} key points is more than one call takes (B <= 65535, B L < 2^31)")
    # ---- nothing above touches the device
    depth0, depth1 = _device_tensor(depth0, names[0]).contiguous(), _device_tensor(depth1, names[1]).contiguous()
    dev = depth0.device
    if kpts is not None:
        kpts = _device_tensor(kpts, "kpts0").contiguous()
    T, K0, K1 = _small(T, names[2], dev), _small(K0, names[3], dev), _small(K1, names[4], dev)
    valid = torch.empty((B, L), device=dev, dtype=torch.bool) if want_valid else None
    prob = torch.empty((B, L), device=dev, dtype=torch.float32) if want_prob else None
    rel = torch.empty((B, L), device=dev, dtype=torch.float64) if want_rel else None
    warped = torch.empty((B, L, 2), device=dev, dtype=torch.float64)
    if B > 0 and L > 0:
        gh, gw = (0, 0) if kpts is not None else grid_hw
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_warp_kpts(
                _ptr(kpts), int(kpts is not None and kpts.dtype == torch.float64), gh, gw, _ptr(depth0), _ptr(depth1), _ptr(T),
                int(T.shape[1]), _ptr(K0), _ptr(K1), B, L, int(depth0.shape[1]), int(depth0.shape[2]), int(depth1.shape[1]),
                int(depth1.shape[2]), thr, _ptr(valid), _ptr(prob), _ptr(rel), _ptr(warped), _stream(dev)))
    return valid, prob, rel, warped


def warp_kpts(kpts0, depth0, depth1, T_0to1, K0, K1, smooth_mask=False, return_relative_depth_error=False,
              depth_interpolation_mode="bilinear", relative_depth_error_threshold=0.05):
    """The reference's `warp_kpts` on the device (`roma_op_warp_kpts`): key points of image 0 moved into image 1 through sensor depth,
    with the covisibility and relative-depth-consistency checks.  kpts0 [B, L, 2] normalised, float32 or float64 (read in place);
    depth0 [B, H0, W0], depth1 [B, H1, W1] float32 (the sizes may differ); T_0to1 [B, 3, 4] or [B, 4, 4]; K0, K1 [B, 3, 3] - device
    tensors, or numpy for the three small ones.

    Returns (valid bool [B, L], warped float64 [B, L, 2]); with return_relative_depth_error=True (rel float64 [B, L], warped) -
    the reference's shapes and dtypes.  warped is written for every row, valid or not; rel is inf where the sampled depth is 0
    and NaN for 0 / 0.  Only depth_interpolation_mode="bilinear" and a falsy smooth_mask are implemented."""
    _mode(depth_interpolation_mode, smooth_mask)
    thr = _threshold(relative_depth_error_threshold)
    want_rel = bool(return_relative_depth_error)
    valid, _, rel, warped = _warp(kpts0, None, depth0, depth1, T_0to1, K0, K1, thr, not want_rel, False, want_rel,
                                  ("depth0", "depth1", "T_0to1", "K0", "K1"))
    return (rel, warped) if want_rel else (valid, warped)


def get_gt_warp(depth1, depth2, T_1to2, K1, K2, depth_interpolation_mode="bilinear", relative_depth_error_threshold=0.05, H=None,
                W=None):
    """The reference's `get_gt_warp` on the device: `warp_kpts` of the pixel centres of an H x W grid over image 1 (default: depth1's
    size), generated in the kernel - grid value j of n is float32((2 j + 1) / n - 1), the correctly rounded value of what the
    reference's float32 linspace(-1 + 1/n, 1 - 1/n, n) approximates.  Returns (x2 float64 [B, H, W, 2], prob float32 [B, H, W])."""
    _mode(depth_interpolation_mode)
    thr = _threshold(relative_depth_error_threshold)
    _depth_shape(depth1, "depth1")
    if (H is None) != (W is None):
        raise ValueError("roma_amd.gt_warp: H and W must be given together")
    H, W = (int(depth1.shape[1]), int(depth1.shape[2])) if H is None else (int(H), int(W))
    if H < 1 or W < 1 or H > 32768 or W > 32768:
        raise ValueError(f"roma_amd.gt_warp: the grid must lie in [1, 32768]^2, got ({H}, {W})")
    _, prob, _, warped = _warp(None, (H, W), depth1, depth2, T_1to2, K1, K2, thr, False, True, False,
                               ("depth1", "depth2", "T_1to2", "K1", "K2"))
    B = int(depth1.shape[0])
    return warped.reshape(B, H, W, 2), prob.reshape(B, H, W)


def dense_metrics(dense_matches, depth1, depth2, T_1to2, K1, K2, relative_depth_error_threshold=0.05, thresholds=(1.0, 3.0, 5.0),
                  return_maps=False):
    """`MegadepthDenseBenchmark.geometric_dist` in one pass on the device (`roma_op_dense_metrics`): the pixel distance of the
    predicted B coordinates (columns 2:4) of a dense warp to the depth-warped A coordinates (columns 0:2), over the pixels whose
    ground truth is valid.  dense_matches float32 [B, h, w, 4] as `match()` returns it, read in place - also the left half
    `warp[:, :, :w]` of a symmetric warp (any row and batch stride; for the B -> A half call with the roles swapped).  The pixel
    scale is the warp grid's (h, w), not depth2's size, as in the reference.  thresholds: the three PCK distances in pixels.

    Returns DenseMetrics: per pair n_valid int64 [B], n_below int64 [B, 3], gd_sum float64 [B]; per batch epe float64 [] and pck
    float64 [3], the means over all valid pixels of the batch (NaN when there is none); with return_maps=True also prob float32
    [B, h, w] and gd float64 [B, h, w], NaN where prob == 0 (otherwise None)."""
    thr = _threshold(relative_depth_error_threshold)
    pck_thr = tuple(float(x) for x in thresholds)
    if len(pck_thr) != 3 or not all(x >= 0 for x in pck_thr):
        raise ValueError("roma_amd.gt_warp: thresholds must be three distances that are not negative")
    m = dense_matches
    if not isinstance(m, torch.Tensor):
        raise TypeError(f"roma_amd.gt_warp: dense_matches must be a torch tensor, got {type(m).__name__}")
    if m.dim() != 4 or m.shape[-1] != 4 or m.dtype != torch.float32 or min(m.shape[:3]) < 1:
        raise ValueError(f"roma_amd.gt_warp: dense_matches must be float32 [B, h, w, 4] with B, h, w >= 1, got {m.dtype} {tuple(m.shape)}")
    B, h, w = (int(x) for x in m.shape[:3])
    if B > 65535 or h > 32768 or w > 32768 or B * h * w >= 2 ** 31:
        raise ValueError(f"roma_amd.gt_warp: {B} x {h} x {w} pixels is more than one call takes (B <= 65535, h, w <= 32768, B h w < 2^31)")
    _, T, K1, K2 = _pair_shapes(B, depth1, depth2, T_1to2, K1, K2, ("depth1", "depth2", "T_1to2", "K1", "K2"))
    # ---- nothing above touches the device
    m = _device_tensor(m, "dense_matches")
    sb, sr, sc, se = m.stride()
    sc, sr = (4 if w == 1 else sc), (4 * w if h == 1 else sr)  # the stride of an axis of length 1 is never used
    sb = h * sr if B == 1 else sb
    in_place = se == 1 and sc == 4 and sr % 4 == 0 and sb % 4 == 0 and sr >= 4 * w and sb >= (h - 1) * sr + 4 * w and m.data_ptr() % 16 == 0
    if not in_place:
        m = m.contiguous()
        m = m.clone() if m.data_ptr() % 16 else m  # a contiguous view at an odd offset: a fresh allocation is aligned
        sb, sr = 4 * h * w, 4 * w
    depth1, depth2 = _device_tensor(depth1, "depth1").contiguous(), _device_tensor(depth2, "depth2").contiguous()
    dev = m.device
    T, K1, K2 = _small(T, "T_1to2", dev), _small(K1, "K1", dev), _small(K2, "K2", dev)
    lib = _lib.load()
    n_valid = torch.empty((B,), device=dev, dtype=torch.int64)
    n_below = torch.empty((B, 3), device=dev, dtype=torch.int64)
    gd_sum = torch.empty((B,), device=dev, dtype=torch.float64)
    epe = torch.empty((), device=dev, dtype=torch.float64)
    pck = torch.empty((3,), device=dev, dtype=torch.float64)
    prob = torch.empty((B, h, w), device=dev, dtype=torch.float32) if return_maps else None
    gd = torch.empty((B, h, w), device=dev, dtype=torch.float64) if return_maps else None
    ws_bytes = int(lib.roma_op_dense_metrics_workspace(B, h, w))
    if ws_bytes < 0:
        raise _lib.RomaHipError("roma_amd.gt_warp: roma_op_dense_metrics_workspace refused the sizes")
    ws = torch.empty((ws_bytes + 7) // 8, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(lib.roma_op_dense_metrics(
            _ptr(m), int(sb), int(sr), _ptr(depth1), _ptr(depth2), _ptr(T), int(T.shape[1]), _ptr(K1), _ptr(K2), B, h, w,
            int(depth1.shape[1]), int(depth1.shape[2]), int(depth2.shape[1]), int(depth2.shape[2]), thr, *pck_thr, _ptr(n_valid),
            _ptr(n_below), _ptr(gd_sum), _ptr(epe), _ptr(pck), _ptr(prob), _ptr(gd), _ptr(ws), ws_bytes, _stream(dev)))
    return DenseMetrics(n_valid, n_below, gd_sum, epe, pck, prob, gd)
