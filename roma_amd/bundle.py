"""Bundle adjustment on the device (`roma_op_bundle_adjust`, csrc/bundle.hip): cameras and 3-D points refined together on the
reprojection error - the closing step after `estimate_pose` / `triangulate` / `estimate_absolute_pose`, which each fit one
side with the other held.  Batched over independent problems of up to 8 views, one launch, no read-back.

More than two views, from detector keypoints x[v] [K, 2] shared by the pairs (a, b) of V images, nothing read back:

    km = model.match_keypoints(x_a, x_b, warp, cert)                       # one batch entry per pair
    tr = build_tracks(km.inds, pairs, V, match_counts=km.counts, kpts=torch.stack(x))
    rec = reconstruct_views(tr.kpts, K, norm_thresh, reproj_thresh, counts=tr.counts)

`reconstruct_views` seeds on views 0 and 1, registers every further view in one shot against the seed pair's points,
triangulates from all registered views and closes with `bundle_adjust`.

Levenberg-Marquardt with the Schur complement under the truncated loss sum min(|r|^2, thr^2) over the observations; the
constants and the accept / reject / stop rules are those of `refine_pose` (csrc/lm_fit.h).  The algorithm is restated in numpy
float64 by tools/bundle_ref.py.  x_cam = R X + t.
"""
from __future__ import annotations

from functools import partial
from typing import NamedTuple

import torch

from . import _lib
from ._lib import _ptr, _stream
from .geometry import _counts, _valid

MAX_VIEWS = 8  # csrc/bundle.hip: ROMA_BA_MAX_VIEWS


class BundleResult(NamedTuple):
    points: torch.Tensor  # [.., N, 3] float64
    R: torch.Tensor       # [.., V, 3, 3] float64
    t: torch.Tensor       # [.., V, 3] float64
    mask: torch.Tensor    # [.., V, N] bool: the observations inside the threshold under the returned state
    info: torch.Tensor    # [.., 6] int32: accepted steps, cost evaluations, active rows, points adjusted, free camera parameters, fitted
    cost: torch.Tensor    # [.., 2] float64: truncated cost at the start and at the end (normalised image coordinates)


class ViewsReconstruction(NamedTuple):
    R: torch.Tensor        # [.., V, 3, 3] float64, x_cam = R X + t; view 0 is the identity; identity for a view that is not registered
    t: torch.Tensor        # [.., V, 3] float64
    points: torch.Tensor   # [.., N, 3] float64 in view 0's frame, NaN where there is none
    mask: torch.Tensor     # [.., V, N] bool: the observations inside reproj_thresh under the returned state
    view_ok: torch.Tensor  # [.., V] bool: the view is registered
    ok: torch.Tensor       # [..] bool: the seed pair gave a pose
    info: torch.Tensor     # [.., 6] int32: `bundle_adjust`'s
    cost: torch.Tensor     # [.., 2] float64: `bundle_adjust`'s truncated cost at the start and at the end


_device_tensor = partial(_lib._device_tensor, module="bundle")


def _view_cameras(K, B, V, dev):
    """[B, V, 3, 3] float64 device camera matrices, or None (normalised observations)"""
    if K is None:
        return None
    K = torch.as_tensor(K).to(device=dev, dtype=torch.float64)
    if K.shape == (3, 3):
        K = K[None, None].expand(B, V, 3, 3)
    elif K.shape == (V, 3, 3):
        K = K[None].expand(B, V, 3, 3)
    if K.shape != (B, V, 3, 3):
        raise ValueError(f"roma_amd.bundle: K must be [3, 3], [{V}, 3, 3] or [{B}, {V}, 3, 3], got {tuple(K.shape)}")
    return K.contiguous()


def default_hold(t):
    """[B, V, 6] uint8 for translations t [B, V, 3]: view 0 entirely, and of view 1 the translation component of largest magnitude
    in the start, which fixes the scale - the seven parameters a reconstruction is free in"""
    B, V = int(t.shape[0]), int(t.shape[1])
    hold = torch.zeros((B, V, 6), device=t.device, dtype=torch.uint8)
    hold[:, 0] = 1
    if V > 1:
        hold[:, 1].scatter_(1, 3 + t[:, 1].abs().argmax(dim=1, keepdim=True), 1)
    return hold


def bundle_adjust(points3d, kpts, K, R, t, reproj_thresh, max_steps=25, hold=None, counts=None, valid=None):
    """Cameras and points refined together on the reprojection error (roma_op_bundle_adjust): Levenberg-Marquardt with the
    Schur complement under the truncated loss sum min(|r|^2, reproj_thresh^2) over the observations, r = p_xy / z - x_n in
    normalised image coordinates; `refine_absolute_pose`'s residual, threshold rule (divided by (fx + fy) / 2 of the view) and
    loop.  reproj_thresh = inf is plain least squares.  Restated by tools/bundle_ref.py.

    points3d [N, 3] float32 or float64 (`triangulate` returns float32), kpts [V, N, 2] pixels of V <= 8 views (read as float32; a
    non-finite entry: the point is not observed there), K [V, 3, 3] or [3, 3] (None: kpts are normalised image coordinates, and
    so is the threshold), R [V, 3, 3], t [V, 3] or [V, 3, 1] with x_cam = R X + t; or the same with a leading batch axis B
    ([B, N, 3], [B, V, N, 2], [B, V, 3, 3] ...) for B independent problems.  hold [.., V, 6] bool: the camera parameters (three of
    the rotation update R <- exp([w]x) R, three of t) that stay; None holds view 0 entirely and the component of t_1 of largest
    magnitude, which fixes the scale.  counts [B]: the points that belong to each problem (see `ransac`); valid [B] bool: the
    problems to fit, the others come back untouched.

    The fit runs in the caller's frame in float64 and is not centred - a held translation component has to stay a plain
    coordinate - so keep the origin near the cameras.  A point with a non-finite start (what `triangulate` leaves where it has
    no point) or fewer than two observations takes no part and comes back with its input bits.  A fit that cannot move
    returns its input: the truncated cost never rises and no value turns into NaN.  A point with fewer than two rows inside
    the threshold is frozen for a step while its rows stay in the cost, so a step of the normal equations need not lower the
    cost: on data with outliers most cost evaluations are rejected retries and a run often ends in them, not in a short
    step.  And the optimum is that of the noisy observations: a start already within a few 1e-3 of the truth may come back no
    better, or worse, in pose (tools/bundle_ref.py and DESIGN.md section 10 item 14 have figures).  Returns BundleResult(points float64, R, t
    [.., V, 3], mask [.., V, N], info [.., 6] = (accepted steps, cost evaluations, active rows at the end, points adjusted, free
    camera parameters, problem fitted), cost [.., 2] = (start, end)); no host synchronisation."""
    X, x = _device_tensor(points3d, "points3d"), _device_tensor(kpts, "kpts")
    R, t = _device_tensor(R, "R"), _device_tensor(t, "t")
    single = X.dim() == 2
    if X.dim() not in (2, 3) or X.shape[-1] != 3 or x.dim() != X.dim() + 1 or x.shape[-1] != 2:
        raise ValueError(f"roma_amd.bundle: need points3d [N, 3] with kpts [V, N, 2] or [B, N, 3] with [B, V, N, 2], got "
                         f"{tuple(X.shape)} and {tuple(x.shape)}")
    dev = X.device
    X = X.detach().to(torch.float64).contiguous()
    x = x.detach().to(device=dev, dtype=torch.float32).contiguous()
    X, x = (X[None], x[None]) if single else (X, x)
    B, V, N = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    if X.shape[0] != B or X.shape[1] != N:
        raise ValueError(f"roma_amd.bundle: points3d {tuple(points3d.shape)} and kpts {tuple(kpts.shape)} differ in problems or points")
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"roma_amd.bundle: need 1 <= V <= {MAX_VIEWS} views, got {V}")
    if not (reproj_thresh > 0) or int(max_steps) < 0:
        raise ValueError("roma_amd.bundle: need reproj_thresh > 0, max_steps >= 0")
    if R.numel() != B * V * 9 or t.numel() != B * V * 3:
        raise ValueError(f"roma_amd.bundle: R and t must hold {B} x {V} poses, got {tuple(R.shape)} and {tuple(t.shape)}")
    R = R.detach().to(device=dev, dtype=torch.float64).reshape(B, V, 3, 3).contiguous()
    t = t.detach().to(device=dev, dtype=torch.float64).reshape(B, V, 3).contiguous()
    K = _view_cameras(K, B, V, dev)
    if hold is None:
        hold = default_hold(t)
    else:
        hold = torch.as_tensor(hold).to(device=dev)
        if tuple(hold.shape) == (V, 6):
            hold = hold[None].expand(B, V, 6)
        if tuple(hold.shape) != (B, V, 6):
            raise ValueError(f"roma_amd.bundle: hold must be [{V}, 6] or [{B}, {V}, 6], got {tuple(hold.shape)}")
        hold = (hold != 0).to(torch.uint8).contiguous()
    counts, valid = _counts(counts, B, dev), _valid(valid, B, dev)
    mask = torch.zeros((B, V, N), device=dev, dtype=torch.bool)
    info = torch.zeros((B, 6), device=dev, dtype=torch.int32)
    cost = torch.full((B, 2), float("nan"), device=dev, dtype=torch.float64)
    if B == 0 or N == 0:
        out = BundleResult(X.clone(), R.clone(), t.clone(), mask, info, cost)
    else:
        out_X, out_R, out_t = torch.empty_like(X), torch.empty_like(R), torch.empty_like(t)
        lib = _lib.load()
        nws = int(lib.roma_op_bundle_adjust_workspace(B, V, N))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_bundle_adjust(_ptr(X), _ptr(x), _ptr(K), _ptr(R), _ptr(t), _ptr(hold), _ptr(counts), _ptr(valid), B, V,
                                                 N, float(reproj_thresh), int(max_steps), _ptr(out_X), _ptr(out_R), _ptr(out_t),
                                                 _ptr(mask), _ptr(info), _ptr(cost), _ptr(ws), nws, _stream(dev)))
        out = BundleResult(out_X, out_R, out_t, mask, info, cost)
    return BundleResult(*(o[0] for o in out)) if single else out


def reconstruct_pair(kpts_A, kpts_B, K_A, K_B, norm_thresh, reproj_thresh, conf=0.99999, max_iters=1000, seed=None, counts=None,
                     method="ransac", max_steps=25):
    """Two views to a refined reconstruction with nothing read back: `estimate_pose(refine=True)`, `triangulate`, NaN where the
    point is not valid (wrong side of a camera, degenerate), then `bundle_adjust` of the two cameras and the points with A as
    the held identity view and the largest component of t held for the scale.  kpts_A, kpts_B pixel keypoints [N, 2] or
    [B, N, 2]; K_A, K_B their cameras, [3, 3] or one per pair [B, 3, 3]; norm_thresh the RANSAC threshold of `estimate_pose` in normalised coordinates,
    reproj_thresh the bundle adjustment's in pixels; conf, max_iters, seed, counts, method as for `estimate_pose`.

    [B, N, 2] -> (R [B, 3, 3] float64, t [B, 3, 1] float64 (A to B, |t| as `estimate_pose` left it up to the held component),
    points [B, N, 3] float64 in A's frame (NaN where there is none), mask [B, N] bool: the matches inside reproj_thresh in both
    views, ok [B]: `estimate_pose` found a pose); [N, 2] -> (R, t, points, mask), or None without a pose."""
    from .geometry import _cameras, _single, estimate_pose
    from .triangulation import triangulate
    a, b = _device_tensor(kpts_A, "kpts_A"), _device_tensor(kpts_B, "kpts_B")
    single = _single(a)
    a, b = (a[None], b[None]) if single else (a, b)
    B, dev = int(a.shape[0]), a.device
    K_A, K_B = _cameras(K_A, B, dev), _cameras(K_B, B, dev)  # [3, 3] or [B, 3, 3], as estimate_pose takes them
    if K_A is None or K_B is None:
        raise ValueError("roma_amd.bundle: K_A and K_B are required")
    R, t, _, ok = estimate_pose(a, b, K_A, K_B, norm_thresh, conf, max_iters, seed, counts, refine=True, method=method)
    tri = triangulate(a, b, R, t, K_A, K_B, counts=counts, valid=ok)
    nan = torch.full((), float("nan"), device=dev, dtype=torch.float64)
    pts = torch.where(tri.valid[..., None], tri.points.to(torch.float64), nan)
    Rs = torch.stack((torch.eye(3, device=dev, dtype=torch.float64).expand(B, 3, 3), R), dim=1)
    ts = torch.stack((torch.zeros((B, 3), device=dev, dtype=torch.float64), t.reshape(B, 3)), dim=1)
    out = bundle_adjust(pts, torch.stack((a, b), dim=1), torch.stack((K_A, K_B), dim=1), Rs, ts, reproj_thresh, max_steps,
                        counts=counts, valid=ok)
    res = (out.R[:, 1], out.t[:, 1, :, None], out.points, out.mask[:, 0] & out.mask[:, 1])
    if not single:
        return (*res, ok)
    return tuple(r[0] for r in res) if bool(ok[0]) else None


def reconstruct_views(kpts, K, norm_thresh, reproj_thresh, conf=0.99999, max_iters=1000, seed=None, counts=None, method="ransac",
                      max_steps=25, min_parallax=0.0):
    """V views to a refined reconstruction with nothing read back - composition only.  kpts [B, V, N, 2] or [V, N, 2] pixels of
    2 <= V <= 8 views, one row per track, a non-finite entry where the view does not observe it (`build_tracks`' kpts); K
    [V, 3, 3], [3, 3] or [B, V, 3, 3]; norm_thresh the RANSAC threshold of `estimate_pose` in normalised coordinates,
    reproj_thresh in pixels for everything after it; conf and max_iters go to both RANSAC runs (`estimate_pose` on the seed pair
    and `estimate_absolute_pose` on the further views), seed, counts, method as for `estimate_pose`.

      1. `estimate_pose(refine=True)` on views 0 and 1 (rows with a NaN are never inliers)
      2. `triangulate_views` with only views 0 and 1 valid, max_reproj = reproj_thresh; points that are not valid become NaN
      3. one `estimate_absolute_pose(refine=True)` call over the B (V - 2) further views against those points, seeds derived
         from `seed`
      4. `triangulate_views` over all registered views
      5. `bundle_adjust` under the default hold, every view that is not registered held entirely and its observations NaN,
         valid = the seed pair's ok

    Registration is one shot against the seed pair's points: a view that shares no track with views 0 and 1 comes back with
    view_ok false and the identity pose.  Returns ViewsReconstruction(R, t, points, mask, view_ok, ok, info, cost); the
    single-problem form returns everything without the batch axis."""
    from .absolute_pose import estimate_absolute_pose
    from .geometry import _seeds, estimate_pose
    from .triangulation import triangulate_views
    if not isinstance(kpts, torch.Tensor) or kpts.dim() not in (3, 4) or kpts.shape[-1] != 2 or not 2 <= kpts.shape[-3] <= MAX_VIEWS:
        raise ValueError(f"roma_amd.bundle: kpts must be a tensor [V, N, 2] or [B, V, N, 2] with 2 <= V <= {MAX_VIEWS}")
    x = _device_tensor(kpts, "kpts")
    single = x.dim() == 3
    x = x.detach().to(torch.float32)
    x = (x[None] if single else x).contiguous()
    B, V, N, dev = int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), x.device
    K = _view_cameras(K, B, V, dev)
    if K is None:
        raise ValueError("roma_amd.bundle: K is required")
    counts, seeds = _counts(counts, B, dev), _seeds(seed, B, dev)
    f64 = dict(device=dev, dtype=torch.float64)
    eye, nan = torch.eye(3, **f64), torch.full((), float("nan"), **f64)
    R1, t1, _, ok = estimate_pose(x[:, 0], x[:, 1], K[:, 0], K[:, 1], norm_thresh, conf, max_iters, seeds, counts, refine=True, method=method)
    view_ok = torch.zeros((B, V), device=dev, dtype=torch.bool)
    view_ok[:, :2] = ok[:, None]
    Rs = eye.expand(B, V, 3, 3).clone()
    ts = torch.zeros((B, V, 3), **f64)
    Rs[:, 1], ts[:, 1] = R1, t1.reshape(B, 3)
    if V > 2:
        tri = triangulate_views(x, K, Rs, ts, view_valid=view_ok, counts=counts, valid=ok, max_reproj=reproj_thresh, min_parallax=min_parallax)
        pts = torch.where(tri.valid[..., None], tri.points, nan)
        more = V - 2
        Xr = pts[:, None].expand(B, more, N, 3).reshape(B * more, N, 3)
        step = torch.arange(1, more + 1, device=dev, dtype=torch.int64) * 1000003
        Rr, tr, _, okr = estimate_absolute_pose(Xr, x[:, 2:].reshape(B * more, N, 2), K[:, 2:].reshape(B * more, 3, 3), reproj_thresh,
                                                conf=conf, max_iters=max_iters, seed=(seeds[:, None] + step).reshape(-1),
                                                counts=None if counts is None else counts.repeat_interleave(more), refine=True,
                                                max_steps=max_steps)
        view_ok = torch.cat((view_ok[:, :2], okr.reshape(B, more) & ok[:, None]), dim=1)
        Rs = torch.cat((Rs[:, :2], Rr.reshape(B, more, 3, 3)), dim=1)
        ts = torch.cat((ts[:, :2], tr.reshape(B, more, 3)), dim=1)
    Rs = torch.where(view_ok[..., None, None], Rs, eye).contiguous()
    ts = torch.where(view_ok[..., None], ts, torch.zeros((), **f64)).contiguous()
    tri = triangulate_views(x, K, Rs, ts, view_valid=view_ok, counts=counts, valid=ok, max_reproj=reproj_thresh, min_parallax=min_parallax)
    pts = torch.where(tri.valid[..., None], tri.points, nan)
    hold = default_hold(ts) | (~view_ok[..., None]).to(torch.uint8)
    seen = torch.where(view_ok[:, :, None, None], x, torch.full((), float("nan"), device=dev, dtype=torch.float32))
    out = bundle_adjust(pts, seen, K, Rs, ts, reproj_thresh, max_steps, hold=hold, counts=counts, valid=ok)
    res = ViewsReconstruction(out.R, out.t, out.points, out.mask, view_ok, ok, out.info, out.cost)
    return ViewsReconstruction(*(r[0] for r in res)) if single else res
