"""`RegressionMatcher.match_keypoints` (romatch/models/matcher.py:732-773) for a whole batch of warps on the device
(`roma_op_match_keypoints`, csrc/keypoints_batched.hip): detector keypoints of B image pairs, each pair with its own warp,
certainty and keypoint counts, matched as mutual nearest neighbours through the warp in one enqueue of five launches - no loop
over pairs, no host read - and returned padded and counted, so that the result feeds the batched geometry through `counts=`.
The definition is stated in include/roma_hip.h and restated in numpy float32 by tools/keypoints_ref.py.

Conventions are those of `roma_amd.sampling.sample_matches`: device tensors only, nothing synchronises with the host, and a
pair's result is bit-identical from run to run and independent of the batch it sits in."""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from . import _lib
from ._lib import _ptr, _stream

MAX_POINTS = 1 << 20  # keypoints per pair and side that one call takes

KeypointMatches = namedtuple("KeypointMatches", "kpts_A kpts_B inds counts total")
KeypointMatches.__doc__ = """kpts_A, kpts_B [B, M, 2] float32 (the matched rows of x_A / x_B, in pixels with `sizes`), inds [B, M, 2]
int32 (index into x_A, index into x_B; -1 beyond counts), counts [B] int32 = min(total, M) leading rows that are matches, total [B]
int64 = the pair's number of mutual matches.  Without a batch axis in the single-pair form."""


def _counts(counts, name, B, single):
    if counts is None:
        return None
    if single:
        raise ValueError(f"roma_amd.match_keypoints: {name} belongs to the batched form; slice the keypoints of a single pair instead")
    if not isinstance(counts, torch.Tensor):
        raise TypeError(f"roma_amd.match_keypoints: {name} must be a torch tensor, got {type(counts).__name__}")
    if counts.dtype not in (torch.int32, torch.int64) or tuple(counts.shape) != (B,):
        raise ValueError(f"roma_amd.match_keypoints: {name} must be an int32 or int64 [{B}] tensor, got {counts.dtype} {tuple(counts.shape)}")
    return counts


def _sizes(sizes, B):
    """sizes as (tensor or 4 host floats, is_tensor) after its shape check"""
    if sizes is None:
        return None
    if isinstance(sizes, torch.Tensor):
        if tuple(sizes.shape) != (B, 4) or sizes.dtype == torch.bool or sizes.is_complex():
            raise ValueError(f"roma_amd.match_keypoints: sizes must be (H_A, W_A, H_B, W_B) or a [{B}, 4] tensor, got {tuple(sizes.shape)}")
        return sizes
    try:
        vals = [float(v) for v in sizes]
    except TypeError:
        raise TypeError("roma_amd.match_keypoints: sizes must be (H_A, W_A, H_B, W_B) or a [B, 4] tensor") from None
    if len(vals) != 4 or not all(math.isfinite(v) and v > 0 for v in vals):
        raise ValueError(f"roma_amd.match_keypoints: sizes must be four positive numbers (H_A, W_A, H_B, W_B), got {sizes}")
    return vals


def match_keypoints(x_A, x_B, warp, certainty, counts_A=None, counts_B=None, max_dist=0.005, cert_th=0, max_matches=None, sizes=None,
                    symmetric=False, _stages=False):
    """Mutual-nearest-neighbour matching of detector keypoints through the dense warp, for every pair of a batch in one enqueue.

    x_A [B, NA, 2], x_B [B, NB, 2]  normalised (x, y) keypoints, padded to common widths; pair b uses its first counts_A[b] /
                                    counts_B[b] rows (int32 or int64 [B] device tensors; None: all rows).  Rows at or beyond the
                                    counts are never read.  A pair may have no keypoints at all.
    warp [B, H, W, 4], certainty [B, H, W]  as `match()` returns them; any row and batch stride is read in place, and with
                                    symmetric=True the A -> B half `warp[:, :, :W]` of a symmetric [B, H, 2W, 4] warp (certainty
                                    [B, H, 2W]) is taken as a view.
    max_dist, cert_th               the reference's thresholds: a pair needs certainty > cert_th at the keypoint of A and a
                                    distance below max_dist (normalised units) between the warped keypoint and its match.
    max_matches                     M, the rows of the output (default max(NA, NB)).  Duplicate keypoints tie and every tied pair
                                    is returned, as the reference's torch.nonzero does, so a pair can have more matches than
                                    keypoints: `total` tells, and only the first M in row-major order are written.
    sizes                           (H_A, W_A, H_B, W_B) as numbers, or a [B, 4] tensor: keypoints come out in pixels, the bits
                                    `to_pixel_coordinates` computes.

    Returns `KeypointMatches(kpts_A, kpts_B, inds, counts, total)`: the matched rows of x_A and x_B [B, M, 2], their indices
    [B, M, 2] int32 (row-major: index into A ascending, then index into B), counts [B] int32 = min(total, M) and total [B] int64.
    Rows at or beyond counts[b] hold 0 and -1.  The single-pair form x_A [na, 2], x_B [nb, 2], warp [H, W, 4], certainty [H, W]
    returns the same without the batch axis.

        warp, certainty = model.match(im_A, im_B)                                   # [B, H, 2W, 4], [B, H, 2W] (symmetric)
        m = roma_amd.match_keypoints(x_A, x_B, warp, certainty, counts_A, counts_B, sizes=(H_A, W_A, H_B, W_B), symmetric=True)
        F, mask, ok = roma_amd.find_fundamental(m.kpts_A, m.kpts_B, counts=m.counts)
    """
    for t, name in ((x_A, "x_A"), (x_B, "x_B"), (warp, "warp"), (certainty, "certainty")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"roma_amd.match_keypoints: {name} must be a torch tensor, got {type(t).__name__}")
    single = x_A.dim() == 2
    d = 2 if single else 3
    if x_A.dim() != d or x_B.dim() != d or x_A.shape[-1] != 2 or x_B.shape[-1] != 2 or not x_A.dtype.is_floating_point or not x_B.dtype.is_floating_point:
        raise ValueError("roma_amd.match_keypoints: x_A and x_B must be floating-point [B, NA, 2] and [B, NB, 2] (or [na, 2] and [nb, 2]), got "
                         f"{x_A.dtype} {tuple(x_A.shape)} and {x_B.dtype} {tuple(x_B.shape)}")
    if warp.dim() != d + 1 or warp.shape[-1] != 4 or warp.dtype != torch.float32 or min(warp.shape) < 1:
        raise ValueError(f"roma_amd.match_keypoints: warp must be float32 [B, H, W, 4] ([H, W, 4] for a single pair), got {warp.dtype} {tuple(warp.shape)}")
    if certainty.dtype != torch.float32 or tuple(certainty.shape) != tuple(warp.shape[:-1]):
        raise ValueError(f"roma_amd.match_keypoints: certainty must be float32 {list(warp.shape[:-1])}, got {certainty.dtype} {tuple(certainty.shape)}")
    if single:
        x_A, x_B, warp, certainty = x_A[None], x_B[None], warp[None], certainty[None]
    B, NA, NB = int(x_A.shape[0]), int(x_A.shape[1]), int(x_B.shape[1])
    if B < 1 or int(x_B.shape[0]) != B or int(warp.shape[0]) != B:
        raise ValueError(f"roma_amd.match_keypoints: x_A, x_B and warp must share a batch axis B >= 1, got {tuple(x_A.shape)}, {tuple(x_B.shape)}, {tuple(warp.shape)}")
    if symmetric:
        if warp.shape[2] % 2:
            raise ValueError(f"roma_amd.match_keypoints: a symmetric warp is [B, H, 2W, 4], got {tuple(warp.shape)}")
        half = int(warp.shape[2]) // 2
        warp, certainty = warp[:, :, :half], certainty[:, :, :half]
    H, W = int(warp.shape[1]), int(warp.shape[2])
    counts_A, counts_B = _counts(counts_A, "counts_A", B, single), _counts(counts_B, "counts_B", B, single)
    sizes = _sizes(sizes, B)
    max_dist, cert_th = float(max_dist), float(cert_th)
    if math.isnan(max_dist) or math.isnan(cert_th):
        raise ValueError("roma_amd.match_keypoints: max_dist or cert_th is NaN")
    M = max(NA, NB, 1) if max_matches is None else int(max_matches)
    if M < 1 or M > 2 ** 31 - 1:
        raise ValueError(f"roma_amd.match_keypoints: max_matches must lie in [1, 2^31 - 1], got {max_matches}")
    if B > 65535 or max(NA, NB) > MAX_POINTS or max(H, W) > 32768:
        raise ValueError(f"roma_amd.match_keypoints: B = {B}, NA = {NA}, NB = {NB}, warp {H} x {W} is more than one call takes "
                         f"(B <= 65535, keypoints <= {MAX_POINTS} per side, sides <= 32768)")
    # ---- nothing above touches the device
    tensors = [x_A, x_B, warp, certainty, counts_A, counts_B] + ([sizes] if isinstance(sizes, torch.Tensor) else [])
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.RomaHipError("roma_amd.match_keypoints: tensors must live on a HIP device; there is no CPU fallback")
    dev = warp.device
    if any(t is not None and t.device != dev for t in tensors):
        raise ValueError("roma_amd.match_keypoints: the tensors live on different devices")
    xa = x_A.detach().to(torch.float32).contiguous()
    xb = x_B.detach().to(torch.float32).contiguous()
    ca = counts_A.detach().to(torch.int32).contiguous() if counts_A is not None else None
    cb = counts_B.detach().to(torch.int32).contiguous() if counts_B is not None else None
    warp, certainty = warp.detach(), certainty.detach()
    sb, sr, sc, se = warp.stride()
    sc, sr = (4 if W == 1 else sc), (4 * W if H == 1 else sr)  # the stride of an axis of length 1 is never used
    sb = H * sr if B == 1 else sb
    in_place = se == 1 and sc == 4 and sr % 4 == 0 and sb % 4 == 0 and sr >= 4 * W and sb >= (H - 1) * sr + 4 * W and warp.data_ptr() % 16 == 0
    if not in_place:
        warp = warp.contiguous()
        warp = warp.clone() if warp.data_ptr() % 16 else warp  # a contiguous view at an odd offset: a fresh allocation is aligned
        sb, sr = 4 * H * W, 4 * W
    tb, tr, tc = certainty.stride()
    tr = W if H == 1 else tr
    tb = H * tr if B == 1 else tb
    if not ((tc == 1 or W == 1) and tr >= W and tb >= (H - 1) * tr + W):
        certainty = certainty.contiguous()
        tb, tr = H * W, W
    sz, sz_stride = None, 0
    if isinstance(sizes, torch.Tensor):
        sz, sz_stride = sizes.detach().to(torch.float32).contiguous(), 4
    elif sizes is not None:
        sz = torch.tensor([sizes], dtype=torch.float32).to(dev)  # one small upload, no synchronisation
    lib = _lib.load()
    ws_bytes = int(lib.roma_op_match_keypoints_workspace(B, NA, NB))
    if ws_bytes < 0:
        raise _lib.RomaHipError("roma_amd.match_keypoints: roma_op_match_keypoints_workspace refused the sizes")
    ws = torch.empty((max(ws_bytes, 16),), device=dev, dtype=torch.uint8)
    inds = torch.empty((B, M, 2), device=dev, dtype=torch.int32)
    kpts_A = torch.empty((B, M, 2), device=dev, dtype=torch.float32)
    kpts_B = torch.empty((B, M, 2), device=dev, dtype=torch.float32)
    counts = torch.empty((B,), device=dev, dtype=torch.int32)
    total = torch.empty((B,), device=dev, dtype=torch.int64)
    with torch.cuda.device(dev):
        _lib.check(lib.roma_op_match_keypoints(
            _ptr(xa if NA else None), _ptr(xb if NB else None), _ptr(ca), _ptr(cb), _ptr(warp), int(sb), int(sr), _ptr(certainty), int(tb),
            int(tr), _ptr(sz), sz_stride, B, NA, NB, H, W, max_dist, cert_th, M, _ptr(inds), _ptr(kpts_A), _ptr(kpts_B), _ptr(counts),
            _ptr(total), _ptr(ws), ws_bytes, _stream(dev)))
    out = KeypointMatches(kpts_A, kpts_B, inds, counts, total)
    if single:
        out = KeypointMatches(*(o[0] for o in out))
    if not _stages:
        return out
    # the sampled keypoints and certainties at the head of the workspace, for the tests of the stages
    p_bytes = B * NA * 8
    c_at = (p_bytes + 15) // 16 * 16
    p = ws[:p_bytes].view(torch.float32).view(B, NA, 2)
    c = ws[c_at:c_at + B * NA * 4].view(torch.float32).view(B, NA)
    return out, (p[0], c[0]) if single else (p, c)
