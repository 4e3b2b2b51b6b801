"""Multi-view tracks on the device (`roma_op_build_tracks`, csrc/tracks.hip): pairwise index matches over the pairs of V <= 8
images, joined into tracks - one keypoint per view - and laid out as the [V, N] observation table `triangulate_views`,
`reconstruct_views` and `bundle_adjust` read.  One launch for a batch of problems, nothing read back.

The whole chain for V images with a matcher `model` alone - RoMa is detector-free, so the keypoints are made from the matches
(`roma_amd.keypoints_from_matches`; `model.reconstruct_image_set(images, K, norm_thresh, reproj_thresh)` is these lines):

    warp, cert, pairs = model.match_image_set(images)                      # all i < j, each image encoded once
    kp, counts = model.set_keypoints(warp, cert, pairs, sizes, num=5000)   # sizes: (H, W) per image
    tr = build_tracks(kp.inds, pairs, V, match_counts=counts, num_kpts=kp.num_kpts, kpts=kp.kpts)
    rec = reconstruct_views(tr.kpts, K, norm_thresh, reproj_thresh, counts=tr.counts)

and with a detector's keypoints x[v] [K, 2] (pixels), matched through the warp by `match_keypoints`:

    pairs = [(a, b) for a in range(V) for b in range(a + 1, V)]
    warp, cert = model.match(torch.stack([im[a] for a, b in pairs]), torch.stack([im[b] for a, b in pairs]))
    km = model.match_keypoints(torch.stack([x[a] for a, b in pairs]), torch.stack([x[b] for a, b in pairs]), warp, cert)
    tr = build_tracks(km.inds, pairs, V, match_counts=km.counts, kpts=torch.stack(x))
    rec = reconstruct_views(tr.kpts, K, norm_thresh, reproj_thresh, counts=tr.counts)

A keypoint is the node v K + i; the rows of `inds` are edges; a connected component is a track when it has at least min_views
keypoints and no view twice.  A component that holds two keypoints of one view is dropped whole (the rule of OpenMVG's track
builder).  Tracks are numbered by their smallest node, so the result depends on the set of edges alone: not on the order of the
rows or pairs, on duplicates, or on the schedule.  Restated by tools/tracks_ref.py."""
from __future__ import annotations

from functools import partial
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream

MAX_VIEWS = 8        # csrc/tracks.h: ROMA_TRACKS_MAX_VIEWS
MAX_KPTS = 1 << 16   # ROMA_TRACKS_MAX_KPTS, keypoints per view
MAX_PAIRS = 64       # ROMA_TRACKS_MAX_PAIRS


class Tracks(NamedTuple):
    index: torch.Tensor            # [.., V, T] int32: the keypoint of the track in the view, -1 where it has none and beyond counts
    kpts: Optional[torch.Tensor]   # [.., V, T, 2] float32: that keypoint (NaN where there is none); None without `kpts`
    counts: torch.Tensor           # [..] int32: min(total, T)
    total: torch.Tensor            # [..] int32: the tracks there are
    info: torch.Tensor             # [.., 4] int32: rows used, rows ignored, components of >= 2 keypoints, components dropped


_device_tensor = partial(_lib._device_tensor, module="tracks")


def _pairs(pair_views, V):
    if isinstance(pair_views, torch.Tensor) and pair_views.is_cuda:
        raise ValueError("roma_amd.tracks: pair_views is host data (a list of tuples): it is checked before anything is launched")
    pv = np.ascontiguousarray(np.asarray(pair_views, dtype=np.int32).reshape(-1, 2))
    if len(pv) > MAX_PAIRS:
        raise ValueError(f"roma_amd.tracks: at most {MAX_PAIRS} pairs, got {len(pv)}")
    if len(pv) and (pv.min() < 0 or pv.max() >= V or (pv[:, 0] == pv[:, 1]).any()):
        raise ValueError(f"roma_amd.tracks: pair_views must hold two different views in [0, {V}) per row")
    return pv


def build_tracks(inds, pair_views, num_views, match_counts=None, num_kpts=None, kpts=None, max_tracks=None, min_views=2,
                 kpts_per_view=None):
    """Pairwise index matches to tracks (`roma_op_build_tracks`).  inds [B, P, M, 2] int32 device: row (i, j) of pair p joins
    keypoint i of view pair_views[p][0] to keypoint j of view pair_views[p][1] - `KeypointMatches.inds` with the pairs of one
    problem as its batch axis - or [P, M, 2] for one problem.  pair_views: P tuples of two different views in [0, num_views),
    host data shared by all problems; a pair may occur more than once.  match_counts [B, P]: the rows of each pair that are read
    (`KeypointMatches.counts`; None: all M).  num_kpts [B, V]: the keypoints each view has (None: K each); a row with an index
    outside [0, num_kpts) on either side - the -1 padding of `match_keypoints` - is ignored and counted.  kpts [B, V, K, 2]
    float32 device: the keypoints themselves, in the caller's units; without them kpts_per_view gives K and only the indices
    are returned.

    Returns Tracks(index [B, V, T] int32, kpts [B, V, T, 2] float32 or None, counts [B], total [B], info [B, 4]) with
    T = max_tracks (default K); `total` tells when more tracks exist than were written.  NaN in `kpts` is exactly what
    `triangulate_views` and `bundle_adjust` read as "not observed".  The single-problem form returns everything without the
    batch axis.  No host synchronisation."""
    V = int(num_views)
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError(f"roma_amd.tracks: need 2 <= num_views <= {MAX_VIEWS}, got {V}")
    pv = _pairs(pair_views, V)
    if not isinstance(inds, torch.Tensor) or inds.dim() not in (3, 4) or inds.shape[-1] != 2 or inds.dtype not in (torch.int32, torch.int64):
        raise ValueError("roma_amd.tracks: inds must be an int32 tensor [P, M, 2] or [B, P, M, 2]")
    single = inds.dim() == 3
    B, P, M = (1 if single else int(inds.shape[0])), int(inds.shape[-3]), int(inds.shape[-2])
    if len(pv) != P:
        raise ValueError(f"roma_amd.tracks: {len(pv)} pair_views for {P} pairs of inds")
    if kpts is not None:
        if not isinstance(kpts, torch.Tensor) or tuple(kpts.shape[:-2]) != ((V,) if single else (B, V)) or kpts.shape[-1] != 2:
            raise ValueError(f"roma_amd.tracks: kpts must be [{'' if single else f'{B}, '}{V}, K, 2]")
        K = int(kpts.shape[-2])
    elif kpts_per_view is not None:
        K = int(kpts_per_view)
    else:
        raise ValueError("roma_amd.tracks: without kpts, kpts_per_view must give the keypoints per view K")
    if K < 0 or K > MAX_KPTS:
        raise ValueError(f"roma_amd.tracks: at most {MAX_KPTS} keypoints per view, got {K}")
    T = K if max_tracks is None else int(max_tracks)
    if T < 0 or not 2 <= int(min_views) <= V:
        raise ValueError(f"roma_amd.tracks: need max_tracks >= 0 and 2 <= min_views <= {V}")
    if B * P * M >= 2 ** 30 or B * V * T >= 2 ** 30 or B > 65535:
        raise ValueError("roma_amd.tracks: more than one call takes (B <= 65535, B P M < 2^30, B V max_tracks < 2^30)")
    inds = _device_tensor(inds, "inds")
    dev = inds.device
    inds = inds.detach().to(torch.int32).contiguous().reshape(B, P, M, 2)
    x = None
    if kpts is not None:
        x = _device_tensor(kpts, "kpts").detach().to(device=dev, dtype=torch.float32).contiguous().reshape(B, V, K, 2)

    def ints(t, shape, name):
        if t is None:
            return None
        t = _device_tensor(t, name).detach().to(device=dev, dtype=torch.int32)
        t = t[None] if single and t.dim() == 1 else t
        if tuple(t.shape) != shape:
            raise ValueError(f"roma_amd.tracks: {name} must be {list(shape[1:] if single else shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    match_counts, num_kpts = ints(match_counts, (B, P), "match_counts"), ints(num_kpts, (B, V), "num_kpts")
    index = torch.full((B, V, T), -1, device=dev, dtype=torch.int32)
    out_x = torch.full((B, V, T, 2), float("nan"), device=dev, dtype=torch.float32) if x is not None else None
    counts, total = (torch.zeros((B,), device=dev, dtype=torch.int32) for _ in range(2))
    info = torch.zeros((B, 4), device=dev, dtype=torch.int32)
    if B > 0 and K > 0:
        lib = _lib.load()
        nws = int(lib.roma_op_build_tracks_workspace(B, V, K, P, M))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_build_tracks(_ptr(inds), pv.ctypes.data, _ptr(match_counts), _ptr(num_kpts), _ptr(x), B, V, K, P, M, T,
                                                int(min_views), _ptr(index), _ptr(out_x), _ptr(counts), _ptr(total), _ptr(info), _ptr(ws),
                                                nws, _stream(dev)))
    out = Tracks(index, out_x, counts, total, info)
    return Tracks(*(None if o is None else o[0] for o in out)) if single else out
