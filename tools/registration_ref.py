"""numpy float64 restatement of the device registration (roma_amd/csrc/registration.hip, `roma_amd.registration`): the oracle of
tests/test_gpu_registration.py, pinned by tests/test_cpu_registration.py against SVD Umeyama and exact geometry.  The similarity
y ~ s R x + t between rows (x, y) of corresponding 3-D points.

  closed form   sim3_from_moments: from the count, the centroids, sxx = sum |x - xb|^2 and C = sum (y - yb)(x - xb)^T: Horn's 4 x 4
                symmetric matrix, its largest eigenvector by SWEEPS sweeps of cyclic Jacobi over the pairs (0,1) (0,2) (0,3) (1,2)
                (1,3) (2,3) (`jacobi_rotate`, no convergence test), the rotation of that unit quaternion; Umeyama's scale
                s = <R, C> / sxx (1 without scale); t = yb - s R xb.  No model: fewer than 3 rows, s not finite or not positive,
                the two largest eigenvalues closer than GAP_EPS times the largest.  A three-point sample (`minimal`) is refused
                first when it is collinear in either set: |d12 x d13| < COLLINEAR_EPS |d12| |d13|.
  normalise     x' = sx (x - cx), y' = sy (y - cy): centroids over the rows finite in both sets, scales 1 / mean distance to them;
                without scale sy = sx; the threshold times sy.  Valid with MIN_VALID finite rows and finite scales.
  score         |A x' + t' - y'|^2 < thr'^2 with A = s R (the device in f32, here in f64); a model needs MIN_INLIERS inliers
  rounds        geometry_ref.round_loop with samples of 3 rows and one slot
  refinement    a step is the closed form on the rows active under the current model (r^2 < thr^2; without a start every finite
                row), kept only if the truncated cost sum min(r^2, thr^2) over the finite rows is strictly lower, else the loop
                stops; on the normalised problem
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_ref as gr  # noqa: E402

SAMPLE, SLOTS = 3, 1
SWEEPS = 6             # Jacobi sweeps over the six pairs
COLLINEAR_EPS = 1e-4   # |d12 x d13| / (|d12| |d13|) below which a three-point sample is collinear
GAP_EPS = 1e-8         # (lambda_1 - lambda_2) / lambda_1 of Horn's matrix below which the rotation is free
MIN_ROWS = 3           # rows below which the closed form has no model
MIN_VALID = 4          # finite rows below which a problem is not sampled
MIN_INLIERS = 4        # inliers below which a model is not accepted
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ------------------------------------------------------------------------------------------------------------ the closed form
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def triangle_ok(p):
    """p [M, 3, 3] three points each: |d12 x d13|^2 > eps^2 |d12|^2 |d13|^2"""
    d12, d13 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cr = _cross(d12, d13)
    return _dot(cr, cr) > (COLLINEAR_EPS * COLLINEAR_EPS) * (_dot(d12, d12) * _dot(d13, d13))


def jacobi_rotate(a, v, p, q):
    """one two-sided Jacobi rotation of the symmetric a [M, 4, 4] in the (p, q) plane, accumulated into the columns of v"""
    apq, app, aqq = a[:, p, q].copy(), a[:, p, p].copy(), a[:, q, q].copy()
    th = (aqq - app) / (2.0 * apq)
    tt = np.copysign(1.0, th) / (np.abs(th) + np.sqrt(th * th + 1.0))
    t = np.where(apq != 0.0, tt, 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    a[:, p, p] = app - t * apq
    a[:, q, q] = aqq + t * apq
    a[:, p, q] = 0.0
    a[:, q, p] = 0.0
    for k in range(4):
        if k != p and k != q:
            akp, akq = a[:, k, p].copy(), a[:, k, q].copy()
            a[:, k, p] = a[:, p, k] = c * akp - s * akq
            a[:, k, q] = a[:, q, k] = s * akp + c * akq
        vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
        v[:, k, p] = c * vkp - s * vkq
        v[:, k, q] = s * vkp + c * vkq


def sim3_from_moments(n, xb, yb, sxx, C, with_scale=True):
    """n [M] counts, xb, yb [M, 3] centroids, sxx [M], C [M, 3, 3] = sum (y - yb)(x - xb)^T -> (s [M], R [M, 3, 3], t [M, 3],
    ok [M]); what is returned where ok is False is not meaningful"""
    n, xb, yb, sxx, C = (np.asarray(v, dtype=np.float64) for v in (n, xb, yb, sxx, C))
    m = len(C)
    with np.errstate(all="ignore"):
        # Horn: S_ab = sum x'_a y'_b = C[b, a]
        Sxx, Sxy, Sxz = C[:, 0, 0], C[:, 1, 0], C[:, 2, 0]
        Syx, Syy, Syz = C[:, 0, 1], C[:, 1, 1], C[:, 2, 1]
        Szx, Szy, Szz = C[:, 0, 2], C[:, 1, 2], C[:, 2, 2]
        a = np.zeros((m, 4, 4))
        a[:, 0, 0] = (Sxx + Syy) + Szz
        a[:, 1, 1] = (Sxx - Syy) - Szz
        a[:, 2, 2] = (Syy - Sxx) - Szz
        a[:, 3, 3] = (Szz - Sxx) - Syy
        a[:, 0, 1] = a[:, 1, 0] = Syz - Szy
        a[:, 0, 2] = a[:, 2, 0] = Szx - Sxz
        a[:, 0, 3] = a[:, 3, 0] = Sxy - Syx
        a[:, 1, 2] = a[:, 2, 1] = Sxy + Syx
        a[:, 1, 3] = a[:, 3, 1] = Szx + Sxz
        a[:, 2, 3] = a[:, 3, 2] = Syz + Szy
        v = np.broadcast_to(np.eye(4), (m, 4, 4)).copy()
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                jacobi_rotate(a, v, p, q)
        # the largest eigenvalue (the first on ties), the second largest, the eigenvector
        k = np.zeros(m, dtype=np.int64)
        lam = a[:, 0, 0].copy()
        for j in range(1, 4):
            up = a[:, j, j] > lam
            lam = np.where(up, a[:, j, j], lam)
            k = np.where(up, j, k)
        lam2 = np.full(m, -np.inf)
        for j in range(4):
            lam2 = np.where((j != k) & (a[:, j, j] > lam2), a[:, j, j], lam2)
        q = v[np.arange(m), :, k]
        qn = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        w, x, y, z = q[:, 0] / qn, q[:, 1] / qn, q[:, 2] / qn, q[:, 3] / qn
        R = np.stack([((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                      2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x),
                      2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z], axis=1).reshape(m, 3, 3)
        num = (_dot(R[:, 0], C[:, 0]) + _dot(R[:, 1], C[:, 1])) + _dot(R[:, 2], C[:, 2])
        s = num / sxx if with_scale else np.ones(m)
        ok = (n >= MIN_ROWS) & np.isfinite(s) & (s > 0.0) & ((lam - lam2) > GAP_EPS * lam)
        t = np.stack([yb[:, r] - s * _dot(R[:, r], xb) for r in range(3)], axis=1)
        ok = ok & np.isfinite(t).all(axis=1) & np.isfinite(R).all(axis=(1, 2))
    return s, R, t, ok


def minimal(X, Y, with_scale=True):
    """the models of three-point samples X, Y [M, 3, 3] -> (s [M], R [M, 3, 3], t [M, 3], n [M] in {0, 1}); zeros where n = 0"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    m = len(X)
    if m == 0:
        return np.zeros(0), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, dtype=np.int64)
    with np.errstate(all="ignore"):
        ok = np.isfinite(X).all(axis=(1, 2)) & np.isfinite(Y).all(axis=(1, 2)) & triangle_ok(X) & triangle_ok(Y)
        xb = ((X[:, 0] + X[:, 1]) + X[:, 2]) / 3.0
        yb = ((Y[:, 0] + Y[:, 1]) + Y[:, 2]) / 3.0
        sxx, C = np.zeros(m), np.zeros((m, 3, 3))
        for k in range(3):
            dx, dy = X[:, k] - xb, Y[:, k] - yb
            sxx = sxx + _dot(dx, dx)
            C = C + dy[:, :, None] * dx[:, None, :]
        s, R, t, found = sim3_from_moments(np.full(m, 3.0), xb, yb, sxx, C, with_scale)
    ok = ok & found
    return np.where(ok, s, 0.0), np.where(ok[:, None, None], R, 0.0), np.where(ok[:, None], t, 0.0), ok.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ RANSAC
def normalise(X, Y, thr, with_scale=True):
    """the normalised problem: (x' [n, 3], y' [n, 3], finite rows, (cx, cy, sx, sy), normalised threshold, valid)"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(X).all(axis=1) & np.isfinite(Y).all(axis=1)
        cnt = int(fin.sum())
        cx = X[fin].sum(axis=0) / cnt if cnt else np.zeros(3)
        cy = Y[fin].sum(axis=0) / cnt if cnt else np.zeros(3)
        dx, dy = X - cx, Y - cy
        mx = np.sqrt((dx[fin, 0] ** 2 + dx[fin, 1] ** 2) + dx[fin, 2] ** 2).sum() / cnt if cnt else 0.0
        my = np.sqrt((dy[fin, 0] ** 2 + dy[fin, 1] ** 2) + dy[fin, 2] ** 2).sum() / cnt if cnt else 0.0
        sx = 1.0 / mx if mx > 0 else math.inf
        sy = (1.0 / my if my > 0 else math.inf) if with_scale else sx
        xn = np.where(fin[:, None], dx * sx, np.nan)
        yn = np.where(fin[:, None], dy * sy, np.nan)
    return xn, yn, fin, (cx, cy, sx, sy), thr * sy, math.isfinite(sx) and math.isfinite(sy) and cnt >= MIN_VALID, cnt


def denormalise(nrm, sn, Rn, tn, with_scale=True):
    """the model of the caller's problem: s = s' sx / sy (1 without scale), t = cy + t' / sy - s R cx"""
    cx, cy, sx, sy = nrm
    s = sn * (sx / sy) if with_scale else 1.0
    t = np.array([(cy[r] + tn[r] / sy) - s * ((Rn[r, 0] * cx[0] + Rn[r, 1] * cx[1]) + Rn[r, 2] * cx[2]) for r in range(3)])
    return s, t


def inliers(M, xn, yn, thr):
    """masks [K, n] of the models M [K, 3, 4] = (A | t) of the normalised problem; NaN rows never pass"""
    with np.errstate(invalid="ignore"):
        e = [(((M[:, i, 0, None] * xn[None, :, 0] + M[:, i, 1, None] * xn[None, :, 1]) + M[:, i, 2, None] * xn[None, :, 2])
              + M[:, i, 3, None]) - yn[None, :, i] for i in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] < thr * thr


def ransac(X, Y, thr, conf=0.9999, max_iters=1000, seed=0, with_scale=True):
    """roma_op_align_points for one problem.  Returns a dict: s, R [3, 3], t [3] (zeros without a model), mask [n], ok, rounds,
    best_h, best_root, best (inlier count), valid."""
    xn, yn, fin, nrm, thr_n, valid, _ = normalise(X, Y, thr, with_scale)
    n = len(xn)
    out = dict(s=0.0, R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(n, dtype=bool), ok=False, rounds=0, best_h=-1, best_root=-1,
               best=-1, valid=bool(valid))
    if not valid:
        return out

    def solve(idx):
        s, R, t, nm = minimal(xn[idx], yn[idx], with_scale)
        return np.concatenate([s[:, None, None] * R, t[..., None]], axis=2)[:, None], nm

    _, best, cur, best_h, best_root, rounds = gr.round_loop(
        n, SAMPLE, SLOTS, fin, seed, conf, max_iters, solve, lambda M: (inliers(M, xn, yn, thr_n).sum(axis=1),) * 2, shape=(3, 4))
    out.update(rounds=rounds, best_h=best_h, best_root=best_root, best=best)
    if best < MIN_INLIERS:
        return out
    A, tn = cur[:, :3], cur[:, 3]
    f2 = 0.0
    for e in A.reshape(9):
        f2 = f2 + e * e
    sn = math.sqrt(f2 / 3.0) if with_scale else 1.0
    Rn = A / sn
    s, t = denormalise(nrm, sn, Rn, tn, with_scale)
    out.update(s=s, R=Rn, t=t, mask=inliers(cur[None], xn, yn, thr_n)[0], ok=True)
    return out


# ------------------------------------------------------------------------------------------------------------ refinement
def residual2(s, R, t, x, y):
    """[n] squared residuals |s R x + t - y|^2"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = [(((R[i, 0] * x[:, 0] + R[i, 1] * x[:, 1]) + R[i, 2] * x[:, 2]) * s + t[i]) - y[:, i] for i in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def _cost(model, x, y, fin, thr2):
    """(truncated cost, active rows) of a model (None: every finite row is active, the cost +inf)"""
    r2 = residual2(*model, x, y) if model is not None else np.zeros(len(x))
    with np.errstate(invalid="ignore"):
        act = fin & (r2 < thr2)
    if model is None:
        return math.inf, act, r2
    s = float(r2[act].sum())
    return (s + thr2 * float(fin.sum() - act.sum()) if math.isfinite(thr2) else s), act, r2


def _fit_rows(x, y, act, with_scale):
    """the closed form on the rows `act`: (s, R, t) or None"""
    n = int(act.sum())
    xb, yb = x[act].sum(axis=0) / n, y[act].sum(axis=0) / n
    dx, dy = x[act] - xb, y[act] - yb
    sxx = float(_dot(dx, dx).sum())
    C = (dy[:, :, None] * dx[:, None, :]).sum(axis=0)
    s, R, t, ok = sim3_from_moments([float(n)], xb[None], yb[None], [sxx], C[None], with_scale)
    return (float(s[0]), R[0], t[0]) if ok[0] else None


def fit_loop(model, x, y, fin, thr2, max_steps, with_scale=True, decisions=None):
    """the refinement loop on rows x, y (already normalised, or as they are): (model or None, steps, evals, active rows, cost0,
    cost).  decisions: a list that receives every (candidate cost, current cost) comparison and the squared residuals of every
    model evaluated, for the margin checks of the CPU tests."""
    cur, act, r2 = _cost(model, x, y, fin, thr2)
    if decisions is not None:
        decisions.append(("rows", r2[fin], thr2))
    steps, evals, cost0, nact = 0, 1, cur, int(act.sum()) if model is not None else 0
    while steps < max_steps and int(act.sum()) >= MIN_ROWS:
        cand = _fit_rows(x, y, act, with_scale)
        if cand is None:
            break
        c, act_c, r2 = _cost(cand, x, y, fin, thr2)
        evals += 1
        if decisions is not None:
            decisions.append(("rows", r2[fin], thr2))
            decisions.append(("cost", c, cur))
        if not c < cur:
            break
        model, cur, act, steps, nact = cand, c, act_c, steps + 1, int(act_c.sum())
    return model, steps, evals, (act if model is not None else np.zeros(len(x), dtype=bool)), cost0, cur, nact


def refine(model, X, Y, thr, max_steps=25, with_scale=True, valid=True, decisions=None):
    """roma_amd.refine_similarity for one problem (X, Y what the device reads, i.e. f32-rounded); model (s, R, t) or None.
    Returns a dict: s, R, t (the input - zeros without one - when no step was accepted), mask [n], info = (accepted steps, cost
    evaluations, active rows, problem fitted), cost0, cost (dst's squared units)."""
    xn, yn, fin, nrm, thr_n, _, cnt = normalise(X, Y, thr, with_scale)
    cx, cy, sx, sy = nrm
    n = len(xn)
    if model is not None:
        s0, R0, t0 = float(model[0]), np.array(model[1], dtype=np.float64), np.array(model[2], dtype=np.float64).reshape(3)
    else:
        s0, R0, t0 = 0.0, np.zeros((3, 3)), np.zeros(3)
    ok = bool(valid) and cnt >= MIN_ROWS and math.isfinite(sx) and math.isfinite(sy) and math.isfinite(s0) \
        and bool(np.isfinite(R0).all()) and bool(np.isfinite(t0).all())
    out = dict(s=s0, R=R0, t=t0, mask=np.zeros(n, dtype=bool), info=(0, 0, 0, int(ok)), cost0=math.nan, cost=math.nan)
    if not ok:
        return out
    start = None
    if model is not None:
        tn = np.array([sy * ((s0 * ((R0[r, 0] * cx[0] + R0[r, 1] * cx[1]) + R0[r, 2] * cx[2]) + t0[r]) - cy[r]) for r in range(3)])
        start = (s0 * (sy / sx), R0, tn)
    thr2 = thr_n * thr_n
    got, steps, evals, act, cost0, cur, nact = fit_loop(start, xn, yn, fin, thr2, max_steps, with_scale, decisions)
    out.update(mask=act, info=(steps, evals, nact, 1), cost0=cost0 / (sy * sy), cost=cur / (sy * sy))
    if steps:
        s, t = denormalise(nrm, got[0], got[1], got[2], with_scale)
        out.update(s=s, R=got[1], t=t)
    return out


def align_points(X, Y, thr, with_scale=True, conf=0.9999, max_iters=1000, seed=0, refine_=True, max_steps=25):
    """roma_amd.align_points for one problem: a dict (s, R, t, mask) or None"""
    r = ransac(X, Y, thr, conf, max_iters, seed, with_scale)
    if not r["ok"]:
        return None
    out = dict(s=r["s"], R=r["R"], t=r["t"], mask=r["mask"])
    if refine_:
        o = refine((r["s"], r["R"], r["t"]), X, Y, thr, max_steps, with_scale)
        if o["info"][3]:
            out = dict(s=o["s"], R=o["R"], t=o["t"], mask=o["mask"])
    return out


def fit_similarity(X, Y, with_scale=True):
    """roma_amd.fit_similarity for one problem: every finite row, no truncation, one step"""
    return refine(None, X, Y, math.inf, 1, with_scale)


# ------------------------------------------------------------------------------------------------------------ apply, rows, trajectory
def apply_points(s, R, t, pts):
    """f32 [n, 3] -> f32: s R X + t in f64, rounded once"""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) * s + t[r] for r in range(3)], axis=1).astype(np.float32)


def apply_cameras(s, R, t, cam_R, cam_t):
    """cam_R [V, 3, 3], cam_t [V, 3] -> R_c' = R_c R^T, t_c' = s t_c - R_c' t"""
    cam_R, cam_t = np.asarray(cam_R, dtype=np.float64), np.asarray(cam_t, dtype=np.float64)
    Rn = np.zeros_like(cam_R)
    for p in range(3):
        for q in range(3):
            Rn[:, p, q] = (cam_R[:, p, 0] * R[q, 0] + cam_R[:, p, 1] * R[q, 1]) + cam_R[:, p, 2] * R[q, 2]
    tn = np.stack([s * cam_t[:, p] - ((Rn[:, p, 0] * t[0] + Rn[:, p, 1] * t[1]) + Rn[:, p, 2] * t[2]) for p in range(3)], axis=1)
    return Rn, tn


def apply(s, R, t, points=None, cam_R=None, cam_t=None):
    """roma_amd.apply_similarity for one problem: the moved points, (R', t'), or (points, R', t') when both are given"""
    outs = ([apply_points(s, R, t, points)] if points is not None else []) + (list(apply_cameras(s, R, t, cam_R, cam_t)) if cam_R is not None else [])
    return outs[0] if len(outs) == 1 else tuple(outs)


def _back_project(px, py, d, K, R, t):
    c = [(px - K[0, 2]) / K[0, 0] * d - t[0], (py - K[1, 2]) / K[1, 1] * d - t[1], d - t[2]]
    return np.stack([(R[0, j] * c[0] + R[1, j] * c[1]) + R[2, j] * c[2] for j in range(3)], axis=-1)


def depth_rows(depth_a, depth_b, K, Ra, ta, Rb, tb, step):
    """roma_op_depth_rows for one image: (src [n, 3] f32 in b's world, dst [n, 3] f32 in a's world), NaN rows where either depth
    is non-finite or not positive"""
    da = np.asarray(depth_a, dtype=np.float32).astype(np.float64)[::step, ::step]
    db = np.asarray(depth_b, dtype=np.float32).astype(np.float64)[::step, ::step]
    K, Ra, ta, Rb, tb = (np.asarray(v, dtype=np.float64) for v in (K, Ra, ta, Rb, tb))
    H, W = np.asarray(depth_a).shape
    v, u = np.meshgrid(np.arange(0, H, step), np.arange(0, W, step), indexing="ij")
    px, py = u + 0.5, v + 0.5
    with np.errstate(all="ignore"):
        ok = np.isfinite(da) & np.isfinite(db) & (da > 0) & (db > 0)
        src = np.where(ok[..., None], _back_project(px, py, db, K, Rb, tb.reshape(3)), np.nan)
        dst = np.where(ok[..., None], _back_project(px, py, da, K, Ra, ta.reshape(3)), np.nan)
    return src.reshape(-1, 3).astype(np.float32), dst.reshape(-1, 3).astype(np.float32)


def centres(R, t):
    """camera centres -R^T t of R [V, 3, 3], t [V, 3]"""
    return np.stack([-((R[:, 0, j] * t[:, 0] + R[:, 1, j] * t[:, 1]) + R[:, 2, j] * t[:, 2]) for j in range(3)], axis=1)


def trajectory_error(R, t, R_gt, t_gt, view_ok=None, with_scale=True):
    """roma_amd.trajectory_error for one problem: a dict s, R, t (the fit of the centres to the true ones), centre_err [V],
    rot_err_deg [V], rmse, ok; NaN everywhere without a fit"""
    R, t, R_gt, t_gt = (np.asarray(v, dtype=np.float64) for v in (R, t, R_gt, t_gt))
    V = len(R)
    x, y = centres(R, t), centres(R_gt, t_gt)
    fin = np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1)
    use = fin & (np.ones(V, dtype=bool) if view_ok is None else np.asarray(view_ok, dtype=bool))
    got, steps, *_ = fit_loop(None, x, y, use, math.inf, 1, with_scale)
    nan = dict(s=math.nan, R=np.full((3, 3), np.nan), t=np.full(3, np.nan), centre_err=np.full(V, np.nan),
               rot_err_deg=np.full(V, np.nan), rmse=math.nan, ok=False)
    if steps != 1:
        return nan
    s, Rm, tm = got
    r2 = residual2(s, Rm, tm, x, y)
    Rn, _ = apply_cameras(s, Rm, tm, R, np.zeros((V, 3)))
    M = np.zeros((V, 3, 3))
    for p in range(3):
        for q in range(3):
            M[:, p, q] = (Rn[:, p, 0] * R_gt[:, q, 0] + Rn[:, p, 1] * R_gt[:, q, 1]) + Rn[:, p, 2] * R_gt[:, q, 2]
    a0, a1, a2 = M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]
    sn, cs = 0.5 * np.sqrt((a0 * a0 + a1 * a1) + a2 * a2), 0.5 * (((M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]) - 1.0)
    return dict(s=s, R=Rm, t=tm, centre_err=np.where(fin, np.sqrt(r2), np.nan), rot_err_deg=np.arctan2(sn, cs) * (180.0 / math.pi),
                rmse=math.sqrt(float(r2[use].sum()) / int(use.sum())), ok=True)
