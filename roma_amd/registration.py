"""Registration of 3-D point sets on the device (csrc/registration.hip, declared in include/roma_hip_registration.h): the
similarity (or rigid) transform y ~ s R x + t between rows of corresponding points.  Every reconstruction of this package
lives in a gauge of its own - the origin at its view 0, the scale from its seed pair - so two of them that share views
(`align_points` on the shared tracks' points, or `register_depth_maps` on a shared image, then `apply_similarity`) are joined by
one, and a recovered camera path is scored against ground truth through one (`trajectory_error`).

Three-point RANSAC through the shared pipeline (`align_points`), a closed-form refinement on the truncated loss
(`refine_similarity`), plain Umeyama (`fit_similarity`).  The closed form - Horn's quaternion by a fixed Jacobi schedule,
Umeyama's scale - is restated in numpy float64 by tools/registration_ref.py.  Batched, and nothing is read back in the batched
forms.
"""
from __future__ import annotations

import math
from functools import partial
from typing import NamedTuple

import torch

from . import _lib
from ._lib import _ptr, _stream
from .geometry import _counts, _seeds, _valid

_device_tensor = partial(_lib._device_tensor, module="registration")


class Similarity(NamedTuple):
    """y = scale R x + t: scale [..] float64, R [.., 3, 3] float64, t [.., 3] float64, mask [.., N] bool (the rows within the
    threshold), ok [..] bool, info int32 (`align_points`: [.., 5]; `refine_similarity`, `fit_similarity`: [.., 4])"""
    scale: torch.Tensor
    R: torch.Tensor
    t: torch.Tensor
    mask: torch.Tensor
    ok: torch.Tensor
    info: torch.Tensor


class TrajectoryError(NamedTuple):
    """`trajectory_error`: the fit of the camera centres to the true ones (scale [..], R [.., 3, 3], t [.., 3]), centre_err
    [.., V], rot_err_deg [.., V], rmse [..] over the fitted views, ok [..]; NaN where there is no fit"""
    scale: torch.Tensor
    R: torch.Tensor
    t: torch.Tensor
    centre_err: torch.Tensor
    rot_err_deg: torch.Tensor
    rmse: torch.Tensor
    ok: torch.Tensor


def _rows(src, dst):
    """([B, N, 3] f32, [B, N, 3] f32, single) of the single-problem or batched inputs"""
    x, y = _device_tensor(src, "src"), _device_tensor(dst, "dst")
    for t, name in ((x, "src"), (y, "dst")):
        if t.dim() not in (2, 3) or t.shape[-1] != 3:
            raise ValueError(f"roma_amd.registration: {name} must be [N, 3] or [B, N, 3], got {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"roma_amd.registration: {name} must be float32 or float64, got {t.dtype}")
    if x.shape != y.shape:
        raise ValueError(f"roma_amd.registration: src {tuple(x.shape)} and dst {tuple(y.shape)} differ")
    single = x.dim() == 2
    x = x.to(torch.float32).contiguous()
    y = y.to(device=x.device, dtype=torch.float32).contiguous()
    return (x[None], y[None], True) if single else (x, y, False)


def _f64(v, name, B, shape, dev):
    v = _device_tensor(v, name).to(device=dev, dtype=torch.float64)
    if v.numel() != B * math.prod(shape):
        raise ValueError(f"roma_amd.registration: {name} must hold {B} x {shape}, got {tuple(v.shape)}")
    return v.reshape(B, *shape).contiguous()


def _front(sim, single, none_without_model=False):
    if not single:
        return sim
    if none_without_model and not bool(sim.ok[0]):  # the one host synchronisation of the single-problem form
        return None
    return Similarity(*(v[0] for v in sim))


def _ransac(x, y, thresh, with_scale, conf, max_iters, seed, counts):
    if not (thresh > 0) or not math.isfinite(thresh) or not (0 <= conf <= 1) or int(max_iters) <= 0:
        raise ValueError("roma_amd.registration: need a finite thresh > 0, 0 <= conf <= 1, max_iters > 0")
    B, N, dev = int(x.shape[0]), int(x.shape[1]), x.device
    scale = torch.zeros((B,), device=dev, dtype=torch.float64)
    R = torch.zeros((B, 3, 3), device=dev, dtype=torch.float64)
    t = torch.zeros((B, 3), device=dev, dtype=torch.float64)
    mask = torch.zeros((B, N), device=dev, dtype=torch.bool)
    ok = torch.zeros((B,), device=dev, dtype=torch.bool)
    info = torch.zeros((B, 5), device=dev, dtype=torch.int32)
    if B == 0 or N < 4:  # no problem can hold four rows
        return Similarity(scale, R, t, mask, ok, info)
    counts, seeds = _counts(counts, B, dev), _seeds(seed, B, dev)
    lib = _lib.load()
    nws = int(lib.roma_op_align_points_workspace(B, N))
    ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(lib.roma_op_align_points(_ptr(x), _ptr(y), _ptr(counts), _ptr(seeds), B, N, float(thresh), float(conf),
                                            int(max_iters), int(bool(with_scale)), _ptr(scale), _ptr(R), _ptr(t), _ptr(mask), _ptr(ok),
                                            _ptr(info), _ptr(ws), nws, _stream(dev)))
    return Similarity(scale, R, t, mask, ok, info)


def _refine(start, x, y, thresh, max_steps, with_scale, counts, valid):
    """roma_op_refine_similarity on [B, N, 3] f32 rows: (Similarity with info [B, 4], cost [B, 2]); start (scale, R, t) or None"""
    B, N, dev = int(x.shape[0]), int(x.shape[1]), x.device
    if not (thresh > 0) or int(max_steps) < 0:
        raise ValueError("roma_amd.registration: need thresh > 0 (inf: no truncation), max_steps >= 0")
    if start is not None:
        s0, R0, t0 = _f64(start[0], "scale", B, (), dev), _f64(start[1], "R", B, (3, 3), dev), _f64(start[2], "t", B, (3,), dev)
    else:
        s0 = R0 = t0 = None
    counts, valid = _counts(counts, B, dev), _valid(valid, B, dev)
    scale = torch.zeros((B,), device=dev, dtype=torch.float64) if s0 is None else s0.clone()
    R = torch.zeros((B, 3, 3), device=dev, dtype=torch.float64) if R0 is None else R0.clone()
    t = torch.zeros((B, 3), device=dev, dtype=torch.float64) if t0 is None else t0.clone()
    mask = torch.zeros((B, N), device=dev, dtype=torch.bool)
    info = torch.zeros((B, 4), device=dev, dtype=torch.int32)
    cost = torch.full((B, 2), math.nan, device=dev, dtype=torch.float64)
    if B > 0 and N >= 3:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_refine_similarity(_ptr(s0), _ptr(R0), _ptr(t0), _ptr(x), _ptr(y), _ptr(counts), _ptr(valid),
                                                             B, N, float(thresh), int(max_steps), int(bool(with_scale)), _ptr(scale),
                                                             _ptr(R), _ptr(t), _ptr(mask), _ptr(info), _ptr(cost), _stream(dev)))
    ok = info[:, 3] > 0 if start is not None else info[:, 0] > 0
    return Similarity(scale, R, t, mask, ok, info), cost


def align_points(src, dst, thresh, with_scale=True, conf=0.9999, max_iters=1000, seed=None, counts=None, refine=True, max_steps=25):
    """The similarity y = scale R x + t that takes the points src onto dst, robustly: three-point RANSAC (roma_op_align_points;
    inlier: |scale R x + t - y| < thresh, a distance in dst's units; OpenCV's adaptive iteration count), then refine=True
    `refine_similarity` from the winning sample's model (problems without a model are left alone).  with_scale=False: a rigid
    transform, scale exactly 1.  Both sets are centred and scaled before the f32 scoring, so origin and unit do not matter.  A
    row with a non-finite entry (a track that one reconstruction did not triangulate) is never sampled and never an inlier: no
    compaction is needed.

    src, dst [N, 3] -> `Similarity` (mask [N]), or None when no model was found (fewer than 4 finite rows, no model with 4
    inliers); [B, N, 3] -> `Similarity` with ok [B], and nothing is read back.  info [.., 5] = (rounds run, winning hypothesis,
    its slot, its inlier count, problem valid).  seed: an int, a tensor of B seeds or None (random); counts: [B] rows per
    problem (later rows are never read)."""
    x, y, single = _rows(src, dst)
    sim = _ransac(x, y, thresh, with_scale, conf, max_iters, seed, counts)
    if refine:
        fit, _ = _refine((sim.scale, sim.R, sim.t), x, y, thresh, max_steps, with_scale, counts, sim.ok)
        sim = Similarity(fit.scale, fit.R, fit.t, torch.where(fit.info[:, 3:4] > 0, fit.mask, sim.mask), sim.ok, sim.info)
    return _front(sim, single, none_without_model=True)


def refine_similarity(sim, src, dst, thresh, max_steps=25, with_scale=True, counts=None, valid=None, return_cost=False):
    """Refinement of a similarity under the truncated loss sum min(|r|^2, thresh^2) over the finite rows (roma_op_refine_similarity):
    a step is the closed form on the rows within thresh of the current model and is kept only if the loss is strictly lower;
    otherwise the loop stops, so the loss never rises and a model is never lost.  sim: a `Similarity` or a (scale, R, t) tuple,
    or None - no start: the first step fits every finite row.  thresh=inf: no truncation.  Returns a `Similarity` whose info
    [.., 4] = (accepted steps, loss evaluations, active rows, problem fitted); without an accepted step scale, R, t are the input
    bits (zeros without a start).  ok: the problem was fitted (without a start: a step was accepted).  valid [B] bool marks the
    problems to fit.  return_cost=True: also cost [.., 2], the loss at the start and at the end in dst's squared units."""
    x, y, single = _rows(src, dst)
    start = None if sim is None else (sim[0], sim[1], sim[2])
    fit, cost = _refine(start, x, y, thresh, max_steps, with_scale, counts, valid)
    fit = _front(fit, single)
    return (fit, cost[0] if single else cost) if return_cost else fit


def fit_similarity(src, dst, counts=None, with_scale=True):
    """Plain Umeyama on every finite row, no truncation: `refine_similarity` without a start, thresh=inf, one step.  ok: the rows
    gave a model (at least 3 finite rows, not collinear)."""
    return refine_similarity(None, src, dst, math.inf, 1, with_scale, counts)


def similarity_minimal(X, Y, with_scale=True):
    """The closed form alone on caller-chosen three-point samples: X, Y [S, 3, 3] -> (scale [S], R [S, 3, 3], t [S, 3] float64, n
    [S] int32: 1 where the sample gave a model, else 0 and zeros)."""
    for name, v in (("X", X), ("Y", Y)):
        _device_tensor(v, name)
        if v.dim() != 3 or tuple(v.shape[1:]) != (3, 3):
            raise ValueError(f"roma_amd.registration: {name} must be [S, 3, 3], got {tuple(v.shape)}")
    if X.shape[0] != Y.shape[0]:
        raise ValueError("roma_amd.registration: X and Y differ in the number of samples")
    S, dev = int(X.shape[0]), X.device
    a = X.detach().to(torch.float64).contiguous()
    b = Y.detach().to(device=dev, dtype=torch.float64).contiguous()
    scale = torch.zeros((S,), device=dev, dtype=torch.float64)
    R = torch.zeros((S, 3, 3), device=dev, dtype=torch.float64)
    t = torch.zeros((S, 3), device=dev, dtype=torch.float64)
    n = torch.zeros((S,), device=dev, dtype=torch.int32)
    if S > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_similarity_minimal(_ptr(a), _ptr(b), S, int(bool(with_scale)), _ptr(scale), _ptr(R), _ptr(t),
                                                              _ptr(n), _stream(dev)))
    return scale, R, t, n


def apply_similarity(sim, points=None, R=None, t=None):
    """Move points and cameras by a similarity (roma_op_apply_similarity).  sim: a `Similarity` or (scale, R, t), single or [B].
    points [.., N, 3] float32 -> scale R X + t (float64 arithmetic, rounded once; NaN stays NaN).  Cameras R [.., V, 3, 3],
    t [.., V, 3] (x_cam = R X + t) -> R' = R R_sim^T, t' = scale t - R' t_sim: they see the moved points as before, the scene
    scaled by `scale`.  Returns the moved points, (R', t'), or (points, R', t') when both are given."""
    s0 = _device_tensor(sim[0], "scale")
    single = s0.dim() == 0
    B, dev = (1 if single else int(s0.shape[0])), s0.device
    s0, R0, t0 = _f64(sim[0], "scale", B, (), dev), _f64(sim[1], "R", B, (3, 3), dev), _f64(sim[2], "t", B, (3,), dev)
    if (R is None) != (t is None):
        raise ValueError("roma_amd.registration: camera R and t go together")
    if points is None and R is None:
        raise ValueError("roma_amd.registration: nothing to move: give points, cameras or both")
    p = out_p = cR = ct = out_R = out_t = None
    N = V = 0
    if points is not None:
        p = _device_tensor(points, "points").to(device=dev, dtype=torch.float32)
        p = p[None] if single else p
        if p.dim() != 3 or p.shape[0] != B or p.shape[2] != 3:
            raise ValueError(f"roma_amd.registration: points must be [{'N' if single else f'{B}, N'}, 3], got {tuple(points.shape)}")
        p, N = p.contiguous(), int(p.shape[1])
        out_p = torch.empty_like(p)
    if R is not None:
        cR, ct = _device_tensor(R, "R").to(device=dev, dtype=torch.float64), _device_tensor(t, "t").to(device=dev, dtype=torch.float64)
        cR, ct = (cR[None], ct[None]) if single else (cR, ct)
        if cR.dim() != 4 or cR.shape[0] != B or tuple(cR.shape[2:]) != (3, 3) or ct.numel() != B * cR.shape[1] * 3:
            raise ValueError(f"roma_amd.registration: cameras must be R [.., V, 3, 3], t [.., V, 3], got {tuple(R.shape)}, {tuple(t.shape)}")
        V = int(cR.shape[1])
        cR, ct = cR.contiguous(), ct.reshape(B, V, 3).contiguous()
        out_R, out_t = torch.empty_like(cR), torch.empty_like(ct)
    if B > 0 and (N > 0 or V > 0):
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_apply_similarity(_ptr(s0), _ptr(R0), _ptr(t0), _ptr(p if N else None), N,
                                                            _ptr(cR if V else None), _ptr(ct if V else None), V, B,
                                                            _ptr(out_p if N else None), _ptr(out_R if V else None),
                                                            _ptr(out_t if V else None), _stream(dev)))
    outs = ([out_p] if points is not None else []) + ([out_R, out_t] if R is not None else [])
    outs = [o[0] for o in outs] if single else outs
    return outs[0] if len(outs) == 1 else tuple(outs)


def depth_rows(depth_a, depth_b, K, pose_a, pose_b, step=4):
    """The rows of one image that two reconstructions a and b share (roma_op_depth_rows): every step-th pixel in each direction
    back-projected at its centre through depth_b and pose_b = (R, t) into b's world (src) and through depth_a and pose_a into
    a's world (dst): (src, dst) [.., N, 3] float32, N = ceil(H / step) ceil(W / step), NaN rows where either depth is non-finite
    or not positive.  depth [H, W] or [B, H, W]; K [3, 3] or [B, 3, 3]; poses (R [.., 3, 3], t [.., 3]) with x_cam = R X + t."""
    da, db = _device_tensor(depth_a, "depth_a"), _device_tensor(depth_b, "depth_b")
    if da.dim() not in (2, 3) or da.shape != db.shape:
        raise ValueError(f"roma_amd.registration: depth maps must both be [H, W] or [B, H, W], got {tuple(da.shape)}, {tuple(db.shape)}")
    single = da.dim() == 2
    da = da.to(torch.float32).contiguous()
    db = db.to(device=da.device, dtype=torch.float32).contiguous()
    da, db = (da[None], db[None]) if single else (da, db)
    B, H, W, dev = int(da.shape[0]), int(da.shape[1]), int(da.shape[2]), da.device
    if int(step) < 1 or H <= 0 or W <= 0:
        raise ValueError("roma_amd.registration: need step >= 1 and a non-empty depth map")
    Kd = torch.as_tensor(K).to(device=dev, dtype=torch.float64)
    Kd = Kd[None].expand(B, 3, 3) if Kd.shape == (3, 3) else Kd
    if Kd.shape != (B, 3, 3):
        raise ValueError(f"roma_amd.registration: K must be [3, 3] or [{B}, 3, 3], got {tuple(Kd.shape)}")
    Kd = Kd.contiguous()
    Ra, ta = _f64(pose_a[0], "pose_a R", B, (3, 3), dev), _f64(pose_a[1], "pose_a t", B, (3,), dev)
    Rb, tb = _f64(pose_b[0], "pose_b R", B, (3, 3), dev), _f64(pose_b[1], "pose_b t", B, (3,), dev)
    step = int(step)
    N = ((H + step - 1) // step) * ((W + step - 1) // step)
    src = torch.empty((B, N, 3), device=dev, dtype=torch.float32)
    dst = torch.empty((B, N, 3), device=dev, dtype=torch.float32)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_depth_rows(_ptr(da), _ptr(db), _ptr(Kd), _ptr(Ra), _ptr(ta), _ptr(Rb), _ptr(tb), B, H, W, step,
                                                      _ptr(src), _ptr(dst), _stream(dev)))
    return (src[0], dst[0]) if single else (src, dst)


def register_depth_maps(depth_a, depth_b, K, pose_a, pose_b, thresh, step=4, **align_kw):
    """The similarity that takes reconstruction b into reconstruction a, from one image that both hold with a depth map and a
    pose of their own: `depth_rows`, then `align_points` (its keywords pass through; thresh in a's units)."""
    src, dst = depth_rows(depth_a, depth_b, K, pose_a, pose_b, step)
    return align_points(src, dst, thresh, **align_kw)


def trajectory_error(R, t, R_gt, t_gt, view_ok=None, with_scale=True):
    """The error of a recovered camera path against the true one, up to the similarity between their gauges
    (roma_op_trajectory_error): the centres -R^T t are fitted to the true ones by the closed form over the views view_ok (all
    by default), then per view the distance of the aligned centre to the true one and the angle of the aligned rotation to the
    true one in degrees, and the RMSE over the fitted views.  R [V, 3, 3], t [V, 3] or batched [B, V, ..] -> `TrajectoryError`;
    NaN and ok False for fewer than 3 usable views or collinear centres."""
    Rd = _device_tensor(R, "R")
    if Rd.dim() not in (3, 4) or tuple(Rd.shape[-2:]) != (3, 3):
        raise ValueError(f"roma_amd.registration: R must be [V, 3, 3] or [B, V, 3, 3], got {tuple(Rd.shape)}")
    single = Rd.dim() == 3
    B, V, dev = (1 if single else int(Rd.shape[0])), int(Rd.shape[-3]), Rd.device
    Rd, td = _f64(R, "R", B, (V, 3, 3), dev), _f64(t, "t", B, (V, 3), dev)
    Rg, tg = _f64(R_gt, "R_gt", B, (V, 3, 3), dev), _f64(t_gt, "t_gt", B, (V, 3), dev)
    vo = None
    if view_ok is not None:
        vo = _device_tensor(view_ok, "view_ok").to(device=dev)
        if vo.numel() != B * V:
            raise ValueError(f"roma_amd.registration: view_ok must hold {B} x {V}, got {tuple(vo.shape)}")
        vo = vo.reshape(B, V).to(torch.uint8).contiguous()
    nan = partial(torch.full, fill_value=math.nan, device=dev, dtype=torch.float64)
    scale, Ro, to, ce, re, rmse = nan((B,)), nan((B, 3, 3)), nan((B, 3)), nan((B, V)), nan((B, V)), nan((B,))
    if B > 0 and V > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_trajectory_error(_ptr(Rd), _ptr(td), _ptr(Rg), _ptr(tg), _ptr(vo), B, V, int(bool(with_scale)),
                                                            _ptr(scale), _ptr(Ro), _ptr(to), _ptr(ce), _ptr(re), _ptr(rmse), _stream(dev)))
    out = TrajectoryError(scale, Ro, to, ce, re, rmse, ~torch.isnan(rmse))
    return TrajectoryError(*(v[0] for v in out)) if single else out
