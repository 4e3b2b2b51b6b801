"""numpy float64 restatement of the device absolute pose (roma_amd/csrc/absolute_pose.hip, `roma_amd.absolute_pose`): the
oracle of tests/test_gpu_absolute_pose.py, pinned by exact synthetic geometry in tests/test_cpu_absolute_pose.py.  The camera
pose (R, t) with x_cam = R X + t from rows (X, x): a 3-D point and its image.

  normalise   x_n = ((u - cx) / fx, (v - cy) / fy) (K None: the points are normalised already), the threshold divided by
              (fx + fy) / 2; X' = s (X - c) with c the centroid of the finite rows and s = 1 / their mean distance to it.  The
              pose of the normalised problem is (R, t' = s (R c + t)); the output undoes it, t = t' / s - R c.  A pair is valid
              with at least 4 finite rows and s finite.
  P3P         unit bearings f_i of a sample of three rows, squared sides a2 = |X2 - X3|^2, b2 = |X1 - X3|^2, c2 = |X1 - X2|^2,
              cosines ca = f2.f3, cb = f1.f3, cg = f1.f2, depths s2 = u s1, s3 = v s1.  With A = a2 / b2, C = c2 / b2 the cosine
              laws give  u^2 - 2 ca v u + ((1 - A) v^2 + 2 A cb v - A) = 0  and  u^2 - 2 cg u + Q(v) = 0,
              Q = -C v^2 + 2 C cb v + (1 - C); their difference is u D(v) = N(v), N = (1 - A + C) v^2 + 2 (A - C) cb v + (C - A - 1),
              D = 2 (ca v - cg), and N^2 - 2 cg N D + Q D^2 = 0 is the quartic in v.  Its roots with v > 0: those of p in [0, 1]
              and of the reversed polynomial (w = 1 / v) in [0, 1), each by `unit_roots` - the root of the linear third
              derivative brackets those of the second, those of the first, those of p, every bracket bisected BISECT times -
              then NEWTON Newton steps on p.  Per root: u = N / D (|D| < DEN_EPS: no model), s1 = b / sqrt(1 - 2 cb v + v^2),
              GN Gauss-Newton steps on the three cosine laws in (s1, s2, s3), all three positive, and (R, t) from the
              orthonormal frames of (P2 - P1, (P2 - P1) x (P3 - P1)) in both spaces.  Slots ascend in v.
  score       z = (R X' + t')_z > 0 and |p_xy - x_n z|^2 < thr^2 z^2 (the device in f32, here in f64); a model needs MIN_INLIERS
              inliers: a sample's own three rows always fit each of its solutions
  rounds      geometry_ref.round_loop with samples of 3 rows and SLOTS = 4
  refinement  lm_ref.fit: parameters (w, dt) with R <- exp([w]x) R, t' <- t' + dt; two residuals per row, p_xy / z - x_n; a row
              with z <= 0 or a non-finite value is inactive; on the normalised problem
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_ref as gr  # noqa: E402
import lm_ref  # noqa: E402
from pose_refine_ref import rodrigues  # noqa: E402

SAMPLE, SLOTS = 3, 4
BISECT, NEWTON, GN = 48, 3, 3
DEN_EPS = 1e-9         # |D(v)| below which u = N / D is not formed
COLLINEAR_EPS = 1e-4   # |d12 x d13| / (|d12| |d13|) below which the 3-D sample is collinear
MIN_ROWS = 3           # rows of a pair, and active rows of an iteration, below which nothing is fitted
MIN_VALID = 4          # finite rows below which a pair is not sampled
MIN_INLIERS = 4        # inliers below which a model is not accepted


# ------------------------------------------------------------------------------------------------------------ polynomials
def horner(c, x):
    """c [M, D + 1] ascending powers at x [M]"""
    r = c[:, -1]
    for k in range(c.shape[1] - 2, -1, -1):
        r = r * x + c[:, k]
    return r


def deriv(c):
    return c[:, 1:] * np.arange(1, c.shape[1], dtype=np.float64)


def bisect_level(c, crit):
    """roots of c between the sorted points 0, crit [M, k], 1: one per interval with a sign change, BISECT halvings, the
    interval's right end where there is none (so the row stays sorted): (points [M, k + 1], found [M, k + 1])"""
    m = len(c)
    pts = np.concatenate([np.zeros((m, 1)), crit, np.ones((m, 1))], axis=1)
    out = np.empty((m, pts.shape[1] - 1))
    found = np.zeros(out.shape, dtype=bool)
    for j in range(out.shape[1]):
        x0, x1 = pts[:, j].copy(), pts[:, j + 1].copy()
        n0 = horner(c, x0) < 0
        has = n0 != (horner(c, x1) < 0)
        for _ in range(BISECT):
            mid = 0.5 * (x0 + x1)
            left = (horner(c, mid) < 0) == n0
            x0, x1 = np.where(left, mid, x0), np.where(left, x1, mid)
        out[:, j] = np.where(has, 0.5 * (x0 + x1), pts[:, j + 1])
        found[:, j] = has
    return out, found


def unit_roots(c):
    """roots of the quartics c [M, 5] in [0, 1], ascending: (points [M, 4], found [M, 4])"""
    d1 = deriv(c)
    d2 = deriv(d1)
    d3 = deriv(d2)
    with np.errstate(all="ignore"):
        r = -d3[:, 0] / d3[:, 1]
    crit = np.where(np.isfinite(r) & (r > 0) & (r < 1), r, 1.0)[:, None]
    crit, _ = bisect_level(d2, crit)
    crit, _ = bisect_level(d1, crit)
    return bisect_level(c, crit)


def polymul(a, b):
    out = np.zeros((len(a), a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            out[:, i + j] = out[:, i + j] + a[:, i] * b[:, j]
    return out


# ------------------------------------------------------------------------------------------------------------ P3P
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _frame(p1, p2, p3):
    """orthonormal frames [M, 3 (vector), 3] of (p2 - p1, (p2 - p1) x (p3 - p1)): e1, e2 = e3 x e1, e3"""
    d12, d13 = p2 - p1, p3 - p1
    e1 = d12 / np.sqrt(_dot(d12, d12))[:, None]
    n = _cross(d12, d13)
    e3 = n / np.sqrt(_dot(n, n))[:, None]
    return np.stack([e1, _cross(e3, e1), e3], axis=1)


def p3p(X, x):
    """X [M, 3, 3] points, x [M, 3, 2] normalised image points -> (R [M, 4, 3, 3], t [M, 4, 3], n [M]); solution r < n[i] of
    sample i is (R[i, r], t[i, r]), ascending in v; unused slots are zero"""
    X, x = np.asarray(X, dtype=np.float64), np.asarray(x, dtype=np.float64)
    m = len(X)
    R, t, n = np.zeros((m, SLOTS, 3, 3)), np.zeros((m, SLOTS, 3)), np.zeros(m, dtype=np.int64)
    if m == 0:
        return R, t, n
    with np.errstate(all="ignore"):
        f = np.concatenate([x, np.ones((m, 3, 1))], axis=2)
        f = f / np.sqrt((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2])[..., None]
        X1, X2, X3 = X[:, 0], X[:, 1], X[:, 2]
        d12, d13, d23 = X2 - X1, X3 - X1, X3 - X2
        a2, b2, c2 = _dot(d23, d23), _dot(d13, d13), _dot(d12, d12)
        cr = _cross(d12, d13)
        ok = np.isfinite(X).all(axis=(1, 2)) & np.isfinite(x).all(axis=(1, 2)) \
            & (_dot(cr, cr) > (COLLINEAR_EPS * COLLINEAR_EPS) * (c2 * b2))
        ca, cb, cg = _dot(f[:, 1], f[:, 2]), _dot(f[:, 0], f[:, 2]), _dot(f[:, 0], f[:, 1])
        A, C = a2 / b2, c2 / b2
        N = np.stack([(C - A) - 1.0, (2.0 * (A - C)) * cb, (1.0 - A) + C], axis=1)
        D = np.stack([-2.0 * cg, 2.0 * ca], axis=1)
        Q = np.stack([1.0 - C, (2.0 * C) * cb, -C], axis=1)
        ND = np.concatenate([polymul(N, D), np.zeros((m, 1))], axis=1)
        p = (polymul(N, N) - (2.0 * cg)[:, None] * ND) + polymul(Q, polymul(D, D))
        lo, flo = unit_roots(p)
        hi, fhi = unit_roots(p[:, ::-1])
        fhi = fhi & (hi > 0) & (hi < 1)
        # ascending in v: the roots in [0, 1], then 1 / w for w descending
        vs = np.concatenate([lo, 1.0 / hi[:, ::-1]], axis=1)
        fv = np.concatenate([flo, fhi[:, ::-1]], axis=1) & ok[:, None]
        dp = deriv(p)
        b = np.sqrt(b2)
        Y = np.zeros((m, 3, 3))
        Fw = _frame(X1, X2, X3)
        for j in range(vs.shape[1]):
            v = vs[:, j]
            for _ in range(NEWTON):
                pv, dv = horner(p, v), horner(dp, v)
                v1 = v - pv / dv
                v = np.where(np.isfinite(v1) & (dv != 0), v1, v)
            Dv = horner(D, v)
            u = horner(N, v) / Dv
            s1 = b / np.sqrt((1.0 - (2.0 * cb) * v) + v * v)
            s2, s3 = u * s1, v * s1
            for _ in range(GN):
                F1 = ((s2 * s2 + s3 * s3) - ((2.0 * s2) * s3) * ca) - a2
                F2 = ((s1 * s1 + s3 * s3) - ((2.0 * s1) * s3) * cb) - b2
                F3 = ((s1 * s1 + s2 * s2) - ((2.0 * s1) * s2) * cg) - c2
                j12, j13 = 2.0 * (s2 - s3 * ca), 2.0 * (s3 - s2 * ca)
                j21, j23 = 2.0 * (s1 - s3 * cb), 2.0 * (s3 - s1 * cb)
                j31, j32 = 2.0 * (s1 - s2 * cg), 2.0 * (s2 - s1 * cg)
                # Cramer's rule on [[0, j12, j13], [j21, 0, j23], [j31, j32, 0]] delta = -F
                det = j12 * (j23 * j31) + j13 * (j21 * j32)
                g1, g2, g3 = -F1, -F2, -F3
                e1 = (j12 * (j23 * g3) + j13 * (g2 * j32)) - g1 * (j23 * j32)
                e2 = (j13 * (j21 * g3) + g1 * (j23 * j31)) - j13 * (g2 * j31)
                e3 = (j12 * (g2 * j31) + g1 * (j21 * j32)) - j12 * (j21 * g3)
                n1, n2, n3 = s1 + e1 / det, s2 + e2 / det, s3 + e3 / det
                step = np.isfinite(n1) & np.isfinite(n2) & np.isfinite(n3) & (det != 0)
                s1, s2, s3 = np.where(step, n1, s1), np.where(step, n2, s2), np.where(step, n3, s3)
            good = fv[:, j] & (np.abs(Dv) >= DEN_EPS) & (s1 > 0) & (s2 > 0) & (s3 > 0) \
                & np.isfinite(s1) & np.isfinite(s2) & np.isfinite(s3)
            for k, s in enumerate((s1, s2, s3)):
                Y[:, k] = f[:, k] * s[:, None]
            Fc = _frame(Y[:, 0], Y[:, 1], Y[:, 2])
            Rj = np.zeros((m, 3, 3))
            for r_ in range(3):
                for c_ in range(3):
                    Rj[:, r_, c_] = (Fc[:, 0, r_] * Fw[:, 0, c_] + Fc[:, 1, r_] * Fw[:, 1, c_]) + Fc[:, 2, r_] * Fw[:, 2, c_]
            tj = np.stack([Y[:, 0, r_] - ((Rj[:, r_, 0] * X1[:, 0] + Rj[:, r_, 1] * X1[:, 1]) + Rj[:, r_, 2] * X1[:, 2])
                           for r_ in range(3)], axis=1)
            good = good & np.isfinite(Rj).all(axis=(1, 2)) & np.isfinite(tj).all(axis=1) & (n < SLOTS)
            sel = np.nonzero(good)[0]
            R[sel, n[sel]], t[sel, n[sel]] = Rj[sel], tj[sel]
            n[sel] += 1
    return R, t, n


# ------------------------------------------------------------------------------------------------------------ RANSAC
def normalise(X, x, K, thr):
    """the normalised problem of one pair: (X' [n, 3], x_n [n, 2], finite rows, c, s, normalised threshold, valid)"""
    X, x = np.asarray(X, dtype=np.float64), np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if K is not None:
            K = np.asarray(K, dtype=np.float64)
            x = np.stack([(x[:, 0] - K[0, 2]) / K[0, 0], (x[:, 1] - K[1, 2]) / K[1, 1]], axis=1)
            thr = thr / ((K[0, 0] + K[1, 1]) / 2)
        fin = np.isfinite(X).all(axis=1) & np.isfinite(x).all(axis=1)
        cnt = int(fin.sum())
        c = X[fin].sum(axis=0) / cnt if cnt else np.zeros(3)
        d = X - c
        mean = np.sqrt((d[fin, 0] ** 2 + d[fin, 1] ** 2) + d[fin, 2] ** 2).sum() / cnt if cnt else 0.0
        s = 1.0 / mean if mean > 0 else math.inf
        Xn = np.where(fin[:, None], d * s, np.nan)
        xn = np.where(fin[:, None], x, np.nan)
    return Xn, xn, fin, c, s, thr, cnt >= MIN_VALID and math.isfinite(s)


def inliers(M, Xn, xn, thr):
    """masks [K, n] of the poses M [K, 3, 4] (normalised problem); NaN rows never pass"""
    with np.errstate(invalid="ignore"):
        p = [((M[:, i, 0, None] * Xn[None, :, 0] + M[:, i, 1, None] * Xn[None, :, 1]) + M[:, i, 2, None] * Xn[None, :, 2])
             + M[:, i, 3, None] for i in range(3)]
        z = p[2]
        ex, ey = p[0] - xn[None, :, 0] * z, p[1] - xn[None, :, 1] * z
        return (z > 0) & (ex * ex + ey * ey < (thr * thr) * (z * z))


def residuals(R, t, Xn, xn):
    """[n, 2] reprojection residuals in normalised image coordinates; NaN where z <= 0"""
    with np.errstate(all="ignore"):
        q = Xn @ R.T
        p = q + t
        z = p[:, 2]
        iz = 1.0 / z
        e = np.stack([p[:, 0] * iz - xn[:, 0], p[:, 1] * iz - xn[:, 1]], axis=1)
        return np.where((z > 0)[:, None], e, np.nan)


class AbsPoseFit:
    """the problem as lm_ref.fit takes it: state (R, t'), rows (X', x_n)"""
    MIN_ROWS = MIN_ROWS

    @staticmethod
    def residuals(st, w):
        return residuals(st[0], st[1], w[0], w[1])

    @staticmethod
    def jacobian(st, w):
        R, t = st
        Xn, xn = w
        with np.errstate(all="ignore"):
            q = Xn @ R.T
            p = q + t
            iz = 1.0 / p[:, 2]
            ax, ay = p[:, 0] * iz, p[:, 1] * iz
            e = np.where((p[:, 2] > 0)[:, None], np.stack([ax - xn[:, 0], ay - xn[:, 1]], axis=1), np.nan)
            z0 = np.zeros(len(Xn))
            # dp of the parameters: e_k x q for the rotation, e_k for the translation
            dps = [(z0, -q[:, 2], q[:, 1]), (q[:, 2], z0, -q[:, 0]), (-q[:, 1], q[:, 0], z0),
                   (z0 + 1, z0, z0), (z0, z0 + 1, z0), (z0, z0, z0 + 1)]
            J = np.stack([np.stack([(d[0] - ax * d[2]) * iz for d in dps], axis=1),
                          np.stack([(d[1] - ay * d[2]) * iz for d in dps], axis=1)], axis=1)  # [n, 2, 6]
        return e, J

    @staticmethod
    def normal(J, e, a):
        Ja, ea = J[a], e[a]
        return np.einsum("nri,nrj->ij", Ja, Ja), np.einsum("nri,nr->i", Ja, ea)

    @staticmethod
    def apply(st, d):
        return rodrigues(d[:3]) @ st[0], st[1] + d[3:]


def refine(R, t, X, x, K, thr, max_steps=25, valid=True):
    """roma_amd.refine_absolute_pose for one pair (X, x what the device reads, i.e. f32-rounded).  Returns a dict: R [3, 3],
    t [3], mask [n], info = (accepted steps, cost evaluations, active rows at the end, pair fitted), cost0, cost (normalised)."""
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64).reshape(3)
    Xn, xn, fin, c, s, thr_n, okn = normalise(X, x, K, thr)
    n = len(Xn)
    ok = bool(valid) and n >= MIN_ROWS and okn and np.isfinite(R).all() and np.isfinite(t).all()
    out = dict(R=R, t=t, mask=np.zeros(n, dtype=bool), info=(0, 0, 0, int(ok)), cost0=math.nan, cost=math.nan)
    if not ok:
        return out
    tn = s * (R @ c + t)
    (Rc, tc), steps, evals, a, cost0, cur = lm_ref.fit(AbsPoseFit, (R, tn), (Xn, xn), thr_n, max_steps)
    out.update(mask=a, info=(steps, evals, int(a.sum()), 1), cost0=cost0, cost=cur)
    if steps:
        out.update(R=Rc, t=tc / s - Rc @ c)
    return out


def ransac(X, x, K, thr, conf=0.9999, max_iters=1000, seed=0):
    """roma_op_absolute_pose for one pair.  Returns a dict: R [3, 3], t [3] (zeros without a model), mask [n], ok, rounds,
    best_h, best_root, best (inlier count)."""
    Xn, xn, fin, c, s, thr_n, valid = normalise(X, x, K, thr)
    n = len(Xn)
    out = dict(R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(n, dtype=bool), ok=False, rounds=0, best_h=-1, best_root=-1,
               best=-1, valid=bool(valid))
    if not valid:
        return out

    def solve(idx):
        R, t, nm = p3p(Xn[idx], xn[idx])
        return np.concatenate([R, t[..., None]], axis=3), nm

    _, best, cur, best_h, best_root, rounds = gr.round_loop(
        n, SAMPLE, SLOTS, fin, seed, conf, max_iters, solve, lambda M: (inliers(M, Xn, xn, thr_n).sum(axis=1),) * 2,
        shape=(3, 4))
    out.update(rounds=rounds, best_h=best_h, best_root=best_root, best=best)
    if best < MIN_INLIERS:
        return out
    Rn, tn = cur[:, :3], cur[:, 3]
    out.update(R=Rn, t=tn / s - Rn @ c, mask=inliers(cur[None], Xn, xn, thr_n)[0], ok=True)
    return out


def estimate_absolute_pose(X, x, K=None, reproj_thresh=2.0, conf=0.9999, max_iters=1000, seed=0, refine_=True, max_steps=25):
    """roma_amd.estimate_absolute_pose for one pair: (R, t [3, 1], mask) or None"""
    r = ransac(X, x, K, reproj_thresh, conf, max_iters, seed)
    if not r["ok"]:
        return None
    R, t, mask = r["R"], r["t"], r["mask"]
    if refine_:
        o = refine(R, t, X, x, K, reproj_thresh, max_steps)
        if o["info"][3]:
            R, t, mask = o["R"], o["t"], o["mask"]
    return R, t[:, None].copy(), mask


def lift_matches(matches, depth, K, H_B, W_B):
    """roma_amd.lift_matches for one pair: matches [n, 4] normalised, depth [H, W], K [3, 3] -> (points [n, 3] f32 in camera
    A's frame, kpts_B [n, 2] f32 pixels).  Depth is bilinear (align_corners=False) from four neighbours that are all finite
    and positive, else the point is NaN."""
    m = np.asarray(matches, dtype=np.float32).astype(np.float64)
    d = np.asarray(depth, dtype=np.float32).astype(np.float64)
    K = np.asarray(K, dtype=np.float64)
    H, W = d.shape
    pts = np.full((len(m), 3), np.nan)
    with np.errstate(all="ignore"):
        px, py = (W / 2) * (m[:, 0] + 1.0), (H / 2) * (m[:, 1] + 1.0)
        gx, gy = px - 0.5, py - 0.5
        fx0, fy0 = np.floor(gx), np.floor(gy)
        for i in range(len(m)):
            if not (fx0[i] >= 0 and fx0[i] + 1 <= W - 1 and fy0[i] >= 0 and fy0[i] + 1 <= H - 1):
                continue
            x0, y0 = int(fx0[i]), int(fy0[i])
            d00, d01, d10, d11 = d[y0, x0], d[y0, x0 + 1], d[y0 + 1, x0], d[y0 + 1, x0 + 1]
            if not all(np.isfinite(v) and v > 0 for v in (d00, d01, d10, d11)):
                continue
            ax, ay = gx[i] - fx0[i], gy[i] - fy0[i]
            z = (d00 * (1.0 - ax) + d01 * ax) * (1.0 - ay) + (d10 * (1.0 - ax) + d11 * ax) * ay
            pts[i] = ((px[i] - K[0, 2]) / K[0, 0] * z, (py[i] - K[1, 2]) / K[1, 1] * z, z)
        kb = np.stack([(W_B / 2) * (m[:, 2] + 1.0), (H_B / 2) * (m[:, 3] + 1.0)], axis=1)
    return pts.astype(np.float32), kb.astype(np.float32)
