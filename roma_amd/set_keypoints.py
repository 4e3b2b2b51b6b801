"""Detector-free keypoints on the device (`roma_op_keypoints_from_matches`, csrc/set_keypoints.hip): the dense matches
`sample_batched` draws for the pairs of V <= 8 images, turned into per-view keypoints and index matches - what `build_tracks`
reads when no detector supplies keypoints.  The endpoints pair (i, j) and pair (i, k) put into image i are different continuous
points; here all endpoints that touch a view are quantised to a pixel grid, one keypoint per occupied cell stays (the most
certain endpoint, the earlier row on a tie), keypoints of neighbouring cells closer than `radius` are merged by a
local-maximum test, and every row is re-indexed to the keypoints nearest its endpoints.  The steps are spelled out in
include/roma_hip.h and restated by tools/set_keypoints_ref.py; the result is bit-identical from run to run.  One enqueue for a
batch of problems, nothing read back."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream
from .tracks import MAX_KPTS, MAX_VIEWS, _device_tensor, _pairs

MAX_CELL = 64          # csrc/set_keypoints.hip: SET_KPTS_MAX_CELL
MAX_SIZE = 65535       # SET_KPTS_MAX_SIZE
MAX_GRID = 1 << 22     # SET_KPTS_MAX_GRID, cells of one view
MAX_CELLS = 1 << 28    # SET_KPTS_MAX_CELLS, B (G_total + 1024 V)


class SetKeypoints(NamedTuple):
    kpts: torch.Tensor      # [.., V, K, 2] float32 pixels: the keypoints of every view, NaN at and beyond num_kpts
    score: torch.Tensor     # [.., V, K] float32: the certainty of the endpoint that became the keypoint, 0 beyond num_kpts
    num_kpts: torch.Tensor  # [.., V] int32: min(total, K)
    total: torch.Tensor     # [.., V] int32: the keypoints there are before the cut to K
    inds: torch.Tensor      # [.., P, N, 2] int32: the keypoints of each row's two endpoints, (-1, -1) for a row without
    kept: torch.Tensor      # [.., P] int32: the rows of each pair with indices
    info: torch.Tensor      # [.., 6] int32: rows read, invalid, without a keypoint, dropped by one_to_one, kept; candidates suppressed


def _sizes(sizes, V):
    if isinstance(sizes, torch.Tensor) and sizes.is_cuda:
        raise ValueError("roma_amd.set_keypoints: sizes is host data (a list of (H, W)): it is checked before anything is launched")
    sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64).reshape(-1, 2))
    if len(sz) != V:
        raise ValueError(f"roma_amd.set_keypoints: {len(sz)} sizes for {V} views")
    if sz.min() < 1 or sz.max() > MAX_SIZE:
        raise ValueError(f"roma_amd.set_keypoints: image sizes must lie in [1, {MAX_SIZE}]")
    return sz.astype(np.int32)


def keypoints_from_matches(matches, certainty, pair_views, num_views, sizes, counts=None, cell=2, radius=None, max_kpts=16384,
                           one_to_one=True):
    """Dense matches of an image set to keypoints and index matches (`roma_op_keypoints_from_matches`).  matches [B, P, N, 4]
    float32 device: the normalised (xA, yA, xB, yB) rows `sample_batched` returns, the P pairs of one problem as the second axis,
    or [P, N, 4] for one problem; certainty [B, P, N]; pair_views: P tuples of two different views in [0, num_views), host data;
    sizes: num_views tuples (H, W), host data - the image sizes the intrinsics refer to; counts [B, P] (`sample_batched`'s
    counts; None: all N rows).  cell: the grid in pixels, 1 .. 64; radius: 0 .. cell pixels, None means cell, 0 switches the
    merging of neighbouring cells off (and loses the tracks of points near a cell border); max_kpts K <= 65536; one_to_one: a
    keypoint keeps only its best row within a pair.

    Returns SetKeypoints(kpts [B, V, K, 2], score [B, V, K], num_kpts [B, V], total [B, V], inds [B, P, N, 2], kept [B, P],
    info [B, 6]).  Rows stay where they are, so `counts` serves as `build_tracks`' match_counts:

        kp = keypoints_from_matches(matches, certainty, pairs, V, sizes, counts=counts)
        tr = build_tracks(kp.inds, pairs, V, match_counts=counts, num_kpts=kp.num_kpts, kpts=kp.kpts)

    The single-problem form returns everything without the batch axis.  No host synchronisation."""
    V = int(num_views)
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError(f"roma_amd.set_keypoints: need 2 <= num_views <= {MAX_VIEWS}, got {V}")
    pv = _pairs(pair_views, V)
    sz = _sizes(sizes, V)
    if not isinstance(matches, torch.Tensor) or matches.dim() not in (3, 4) or matches.shape[-1] != 4 or not matches.is_floating_point():
        raise ValueError("roma_amd.set_keypoints: matches must be a float tensor [P, N, 4] or [B, P, N, 4]")
    single = matches.dim() == 3
    B, P, N = (1 if single else int(matches.shape[0])), int(matches.shape[-3]), int(matches.shape[-2])
    if len(pv) != P:
        raise ValueError(f"roma_amd.set_keypoints: {len(pv)} pair_views for {P} pairs of matches")
    if not isinstance(certainty, torch.Tensor) or tuple(certainty.shape) != tuple(matches.shape[:-1]):
        raise ValueError(f"roma_amd.set_keypoints: certainty must be {list(matches.shape[:-1])}")
    cell, K, one_to_one = int(cell), int(max_kpts), bool(one_to_one)
    if not 1 <= cell <= MAX_CELL:
        raise ValueError(f"roma_amd.set_keypoints: cell must lie in [1, {MAX_CELL}] pixels, got {cell}")
    radius = float(cell if radius is None else radius)
    if not 0.0 <= radius <= cell:
        raise ValueError(f"roma_amd.set_keypoints: radius must lie in [0, cell = {cell}], got {radius}")
    if not 1 <= K <= MAX_KPTS:
        raise ValueError(f"roma_amd.set_keypoints: need 1 <= max_kpts <= {MAX_KPTS}, got {K}")
    grids = [((int(h) + cell - 1) // cell) * ((int(w) + cell - 1) // cell) for h, w in sz]
    g_total = sum(grids)
    if max(grids) > MAX_GRID or B * ((g_total + 1023) // 1024 + V) * 1024 > MAX_CELLS:
        raise ValueError(f"roma_amd.set_keypoints: at most {MAX_GRID} cells per view and B (cells + 1024 V) <= {MAX_CELLS}; use a larger cell")
    if 2 * P * N >= 2 ** 32 or B * P * N >= 2 ** 30 or B > 65535:
        raise ValueError("roma_amd.set_keypoints: more than one call takes (B <= 65535, 2 P N < 2^32, B P N < 2^30)")
    matches = _device_tensor(matches, "matches")
    dev = matches.device
    matches = matches.detach().to(torch.float32).contiguous().reshape(B, P, N, 4)
    certainty = _device_tensor(certainty, "certainty").detach().to(device=dev, dtype=torch.float32).contiguous().reshape(B, P, N)
    if counts is not None:
        counts = _device_tensor(counts, "counts").detach().to(device=dev, dtype=torch.int32)
        counts = counts[None] if single and counts.dim() == 1 else counts
        if tuple(counts.shape) != (B, P):
            raise ValueError(f"roma_amd.set_keypoints: counts must be {[P] if single else [B, P]}, got {tuple(counts.shape)}")
        counts = counts.contiguous()
    kpts = torch.full((B, V, K, 2), float("nan"), device=dev, dtype=torch.float32)
    score = torch.zeros((B, V, K), device=dev, dtype=torch.float32)
    num_kpts, total = (torch.zeros((B, V), device=dev, dtype=torch.int32) for _ in range(2))
    inds = torch.full((B, P, N, 2), -1, device=dev, dtype=torch.int32)
    kept = torch.zeros((B, P), device=dev, dtype=torch.int32)
    info = torch.zeros((B, 6), device=dev, dtype=torch.int32)
    if B > 0:
        lib = _lib.load()
        nws = int(lib.roma_op_keypoints_from_matches_workspace(B, V, P, N, g_total, K))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_keypoints_from_matches(_ptr(matches), _ptr(certainty), _ptr(counts), pv.ctypes.data, sz.ctypes.data, B, V,
                                                          P, N, cell, radius, K, int(one_to_one), _ptr(kpts), _ptr(score), _ptr(num_kpts),
                                                          _ptr(total), _ptr(inds), _ptr(kept), _ptr(info), _ptr(ws), nws, _stream(dev)))
    out = SetKeypoints(kpts, score, num_kpts, total, inds, kept, info)
    return SetKeypoints(*(o[0] for o in out)) if single else out
