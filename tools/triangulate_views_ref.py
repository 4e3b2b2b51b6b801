"""numpy float64 restatement of the device N-view triangulation (roma_amd/csrc/triangulate_views.hip, roma_amd.triangulate_views):
the oracle of tests/test_gpu_views.py, itself pinned by exact synthetic geometry in tests/test_cpu_views.py.  One problem at a
time, one point at a time, the same expressions in the same order as the kernel (which is compiled with fp contraction off).

Per point, with the observations in use U (finite, of a valid view, not trimmed), x_n = ((u - cx) / fx, (v - cy) / fy):
  start     fewer than min_views in U: DEGENERATE.  Ray d_v = R_v^T (x_n, 1) / |.| from the centre c_v = -R_v^T t_v; the midpoint
            (sum (I - d d^T)) X = sum (I - d d^T) c by a 3 x 3 Cholesky factor; a pivot that is not finite or not above
            PIVOT_REL x the largest diagonal entry (parallel rays): DEGENERATE
  refine    up to gn_steps Gauss-Newton steps on sum |p_xy / z - x_n|^2, p = R_v X + t_v, over U; a step is kept only when its
            cost is finite and strictly lower, the first one that is not (or whose factor fails) ends the loop
  trim      e_v = |error| / thr_v, thr_v = max_reproj / ((fx_v + fy_v) / 2); when trim is on, the largest e_v is above 1 and U
            holds at least three, the worst observation (the lowest view of a tie) leaves U and the point starts again
"""
from __future__ import annotations

import math

import numpy as np

from lm_ref import PIVOT_REL

SKIPPED, DEGENERATE, CHEIRALITY, REPROJ, PARALLAX = 1, 2, 4, 8, 16
RAD_TO_DEG = 57.29577951308232
F = np.float64


def solve3(A, b):
    """x of A x = b, A the upper triangle (00, 01, 02, 11, 12, 22), or None when a pivot fails"""
    piv = PIVOT_REL * max(max(A[0], A[3]), A[5])
    ok = A[0] > piv and np.isfinite(A[0])
    l00 = np.sqrt(A[0])
    l10, l20 = A[1] / l00, A[2] / l00
    p1 = A[3] - l10 * l10
    ok = ok and p1 > piv and np.isfinite(p1)
    l11 = np.sqrt(p1)
    l21 = (A[4] - l20 * l10) / l11
    p2 = (A[5] - l20 * l20) - l21 * l21
    ok = ok and p2 > piv and np.isfinite(p2)
    if not ok:
        return None
    l22 = np.sqrt(p2)
    y0 = b[0] / l00
    y1 = (b[1] - l10 * y0) / l11
    y2 = ((b[2] - l20 * y0) - l21 * y1) / l22
    x2 = y2 / l22
    x1 = (y1 - l21 * x2) / l11
    x0 = ((y0 - l10 * x1) - l20 * x2) / l00
    return [x0, x1, x2]


class Views:
    """what the kernel stages per view: R (row-major), t, centre, fx, fy, cx, cy, thr, and whether the view takes part"""

    def __init__(self, K, R, t, view_valid, max_reproj):
        V = len(R)
        self.R = np.asarray(R, dtype=F).reshape(V, 9)
        self.t = np.asarray(t, dtype=F).reshape(V, 3)
        self.cam = np.tile(np.array([1.0, 1.0, 0.0, 0.0]), (V, 1))
        self.thr = np.full(V, F(max_reproj))
        self.c = np.zeros((V, 3))
        self.ok = np.ones(V, dtype=bool) if view_valid is None else np.asarray(view_valid).astype(bool).copy()
        with np.errstate(all="ignore"):
            for v in range(V):
                w, tt = self.R[v], self.t[v]
                if K is not None:
                    Kv = np.asarray(K[v], dtype=F)
                    self.cam[v] = (Kv[0, 0], Kv[1, 1], Kv[0, 2], Kv[1, 2])
                    self.thr[v] = F(max_reproj) / ((Kv[0, 0] + Kv[1, 1]) / 2)
                for i in range(3):
                    self.c[v, i] = 0.0 - ((w[i] * tt[0] + w[3 + i] * tt[1]) + w[6 + i] * tt[2])
                self.ok[v] &= bool(np.isfinite(w).all() and np.isfinite(tt).all() and np.isfinite(self.c[v]).all() and np.isfinite(self.cam[v]).all())

    def normalise(self, v, k):
        fx, fy, cx, cy = self.cam[v]
        return (F(k[0]) - cx) / fx, (F(k[1]) - cy) / fy

    def ray(self, v, k):
        x0, x1 = self.normalise(v, k)
        w = self.R[v]
        r0 = (w[0] * x0 + w[3] * x1) + w[6]
        r1 = (w[1] * x0 + w[4] * x1) + w[7]
        r2 = (w[2] * x0 + w[5] * x1) + w[8]
        nrm = np.sqrt((r0 * r0 + r1 * r1) + r2 * r2)
        return [r0 / nrm, r1 / nrm, r2 / nrm]

    def residual(self, v, k, X):
        """(e0, e1, z, 1 / z, ax, ay)"""
        x0, x1 = self.normalise(v, k)
        w, t = self.R[v], self.t[v]
        p = [((w[3 * i] * X[0] + w[3 * i + 1] * X[1]) + w[3 * i + 2] * X[2]) + t[i] for i in range(3)]
        iz = F(1.0) / p[2]
        ax, ay = p[0] * iz, p[1] * iz
        return ax - x0, ay - x1, p[2], iz, ax, ay


def cost(W, kp, use, X, max_depth):
    """(cost, worst error in units of its threshold, its view or -1, cheirality failed) over the views in use"""
    c, worst, wi, cheir = F(0.0), F(0.0), -1, False
    for v in use:
        e0, e1, z, _, _, _ = W.residual(v, kp[v], X)
        e2 = e0 * e0 + e1 * e1
        c = c + e2
        rel = np.sqrt(e2) / W.thr[v]
        if rel > worst:
            worst, wi = rel, v
        if not (z > 0.0 and z < max_depth):
            cheir = True
    return c, worst, wi, cheir


def midpoint(W, kp, use):
    A, b = [F(0.0)] * 6, [F(0.0)] * 3
    for v in use:
        d = W.ray(v, kp[v])
        M = [1.0 - d[0] * d[0], 0.0 - d[0] * d[1], 0.0 - d[0] * d[2], 1.0 - d[1] * d[1], 0.0 - d[1] * d[2], 1.0 - d[2] * d[2]]
        c0, c1, c2 = W.c[v]
        A = [A[q] + M[q] for q in range(6)]
        b = [b[0] + ((M[0] * c0 + M[1] * c1) + M[2] * c2), b[1] + ((M[1] * c0 + M[3] * c1) + M[4] * c2),
             b[2] + ((M[2] * c0 + M[4] * c1) + M[5] * c2)]
    return solve3(A, b)


def gn_step(W, kp, use, X):
    H, g = [F(0.0)] * 6, [F(0.0)] * 3
    for v in use:
        e0, e1, _, iz, ax, ay = W.residual(v, kp[v], X)
        w = W.R[v]
        J0 = [(w[k] - ax * w[6 + k]) * iz for k in range(3)]
        J1 = [(w[3 + k] - ay * w[6 + k]) * iz for k in range(3)]
        q = 0
        for a in range(3):
            for e in range(a, 3):
                H[q] = H[q] + (J0[a] * J0[e] + J1[a] * J1[e])
                q += 1
            g[a] = g[a] + (J0[a] * e0 + J1[a] * e1)
    return solve3(H, [0.0 - g[0], 0.0 - g[1], 0.0 - g[2]])


def triangulate(kpts, K, R, t, view_valid=None, count=None, valid=True, max_reproj=math.inf, min_parallax=0.0, max_depth=math.inf,
                min_views=2, gn_steps=3, trim=True, trace=None):
    """roma_amd.triangulate_views for one problem; kpts [V, N, 2] must hold what the device reads: f32 values.  Returns a dict:
    points [N, 3], reproj [V, N] float32, used [V, N] bool, parallax [N] float32, flags [N] uint8, stats (8 ints), cost0 / cost [N]
    (the midpoint's and the final cost of the last fit).  trace: a list that receives, per trimming decision,
    (point, worst error in threshold units)."""
    kpts = np.asarray(kpts)
    V, N = kpts.shape[:2]
    W = Views(K, R, t, view_valid, max_reproj)
    out = dict(points=np.full((N, 3), np.nan), reproj=np.full((V, N), np.nan, dtype=np.float32), used=np.zeros((V, N), dtype=bool),
               parallax=np.full(N, np.nan, dtype=np.float32), flags=np.full(N, SKIPPED, dtype=np.uint8), cost0=np.full(N, np.nan),
               cost=np.full(N, np.nan))
    stats = [0] * 8
    rows = 0 if not valid else (N if count is None else min(max(int(count), 0), N))
    seen = np.isfinite(kpts).all(axis=2)
    with np.errstate(all="ignore"):
        for j in range(rows):
            stats[0] += 1
            kp = kpts[:, j]
            obs = [v for v in range(V) if W.ok[v] and seen[v, j]]
            use, X, flag, trims = list(obs), None, DEGENERATE, 0
            while True:
                if len(use) < min_views:
                    break
                X = midpoint(W, kp, use)
                if X is None:
                    break
                c, worst, wi, cheir = cost(W, kp, use, X, max_depth)
                out["cost0"][j] = c
                for _ in range(gn_steps):
                    dX = gn_step(W, kp, use, X)
                    if dX is None:
                        break
                    Xn = [X[0] + dX[0], X[1] + dX[1], X[2] + dX[2]]
                    cn, wn, win, chn = cost(W, kp, use, Xn, max_depth)
                    if not (cn < c and np.isfinite(cn)):
                        break
                    X, c, worst, wi, cheir = Xn, cn, wn, win, chn
                out["cost"][j] = c
                if trace is not None:
                    trace.append((j, float(worst)))
                if trim and worst > 1.0 and len(use) >= 3:
                    use.remove(wi)
                    trims += 1
                    continue
                flag = 0
                break
            stats[6] += trims
            if flag:
                stats[2] += 1
                out["flags"][j] = flag
                continue
            dmin, pair = F(np.inf), None
            for a, v in enumerate(use):
                dv = W.ray(v, kp[v])
                for u in use[a + 1:]:
                    du = W.ray(u, kp[u])
                    dot = (dv[0] * du[0] + dv[1] * du[1]) + dv[2] * du[2]
                    if dot < dmin:
                        dmin, pair = dot, (dv, du)
            dv, du = pair
            c0, c1, c2 = dv[1] * du[2] - dv[2] * du[1], dv[2] * du[0] - dv[0] * du[2], dv[0] * du[1] - dv[1] * du[0]
            par = np.arctan2(np.sqrt((c0 * c0 + c1 * c1) + c2 * c2), dmin) * RAD_TO_DEG
            if cheir:
                flag |= CHEIRALITY
                stats[3] += 1
            if worst > 1.0:
                flag |= REPROJ
                stats[4] += 1
            if not par >= min_parallax:
                flag |= PARALLAX
                stats[5] += 1
            stats[1] += flag == 0
            out["points"][j], out["parallax"][j], out["flags"][j] = X, np.float32(par), flag
            out["used"][use, j] = True
            for v in obs:
                e0, e1 = W.residual(v, kp[v], X)[:2]
                ex, ey = W.cam[v, 0] * e0, W.cam[v, 1] * e1
                out["reproj"][v, j] = np.float32(np.sqrt(ex * ex + ey * ey))
    out["stats"] = tuple(int(s) for s in stats)
    return out
