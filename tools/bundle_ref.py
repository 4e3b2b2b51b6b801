"""numpy float64 restatement of the device bundle adjustment (roma_amd/csrc/bundle.hip, roma_amd.bundle_adjust): the oracle of
tests/test_gpu_bundle.py, itself pinned by exact synthetic geometry, by central differences and by the dense solve of the full
damped system in tests/test_cpu_bundle.py.  One problem at a time; the same expressions and the same rules as the kernel, the
constants of tools/lm_ref.py.  Sums over the views of a point run in view order as on the device; sums over points are
numpy's (the device adds them strided over 512 threads), which is what the device tolerance of the tests covers.

  rows      (i, j): point j observed in view i (both pixel coordinates finite); e = p_xy / z - x_n, p = R_i X_j + t_i, active
            when z > 0 and |e|^2 < thr_i^2 with thr_i = thr / ((fx_i + fy_i) / 2); cost = sum min(|e|^2, thr_i^2)
  points    beyond `count`, with a non-finite start or fewer than two observations: not part of the problem; with fewer than
            two active rows or a failed pivot of V_j + lambda diag V_j: frozen for the step (rows in the cost only)
  cameras   a parameter that is held or whose entry of diag U is not positive: unit row, delta exactly 0
  step      S = U + lambda diag U - sum_j W_j Vi_j W_j^T, S dc = -(g_c - sum_j W_j Vi_j g_j), dX_j = Vi_j (-g_j - W_j^T dc)
  stop      max_steps accepted steps, |step| < STEP_TOL, RETRIES failed retries, a failed pivot of S, no free parameter, fewer
            active residuals (two per row) than free parameters
"""
from __future__ import annotations

import math

import numpy as np

from lm_ref import LAMBDA0, LAMBDA_MIN, PIVOT_REL, RETRIES, STEP_TOL

MAX_VIEWS = 8
TRI3 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def rodrigues(w):
    """exp([w]x) as lm_fit.h's lm_rodrigues forms it"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    a, b = 1.0, 0.5
    if not th2 < 1e-30:
        h = 0.5 * math.sqrt(th2)
        sh = math.sin(h) / h
        a, b = sh * math.cos(h), 0.5 * (sh * sh)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return (np.eye(3) + a * K) + b * (K @ K)


def default_hold(t):
    """view 0 entirely, and of view 1 the translation component of largest magnitude in the start: it fixes the scale"""
    V = len(t)
    hold = np.zeros((V, 6), dtype=bool)
    hold[0] = True
    if V > 1:
        hold[1, 3 + int(np.argmax(np.abs(t[1])))] = True
    return hold


def views(K, V, thr):
    """(fx, fy, cx, cy, thr^2) [V, 5] of the views"""
    w = np.zeros((V, 5))
    for i in range(V):
        if K is None:
            w[i] = (1.0, 1.0, 0.0, 0.0, thr * thr)
        else:
            tn = thr / ((K[i, 0, 0] + K[i, 1, 1]) / 2)
            w[i] = (K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2], tn * tn)
    return w


class Problem:
    """the fixed part of one problem: observations, views, hold flags, the points that take part"""

    def __init__(self, X, kpts, K, hold, thr, count=None):
        kpts = np.asarray(kpts)  # as given: the device tests hand over what the device reads, f32 values
        self.V, self.N = kpts.shape[:2]
        self.w = views(None if K is None else np.asarray(K, dtype=np.float64), self.V, thr)
        k = kpts.astype(np.float64)
        self.seen = np.isfinite(kpts).all(axis=2)
        with np.errstate(all="ignore"):
            self.xn = np.stack([(k[..., 0] - self.w[:, 2, None]) / self.w[:, 0, None], (k[..., 1] - self.w[:, 3, None]) / self.w[:, 1, None]], 2)
        n = self.N if count is None else min(max(int(count), 0), self.N)
        self.inc = (np.arange(self.N) < n) & np.isfinite(X).all(axis=1) & (self.seen.sum(axis=0) >= 2)
        self.rows = self.seen & self.inc[None]
        self.hold = np.asarray(hold, dtype=bool).reshape(self.V * 6)
        thr2 = self.w[:, 4]
        self.miss = np.where(np.isfinite(thr2), thr2, 0.0)  # what a row that is not active costs

    def residuals(self, R, t, X):
        """e [V, N, 2], q = R X [V, N, 3], 1 / z, a = p_xy / z, |e|^2 (NaN unless z > 0), active rows [V, N]"""
        with np.errstate(all="ignore"):
            q = np.stack([(R[:, i, 0, None] * X[None, :, 0] + R[:, i, 1, None] * X[None, :, 1]) + R[:, i, 2, None] * X[None, :, 2]
                          for i in range(3)], 2)
            p = q + t[:, None, :]
            iz = 1.0 / p[..., 2]
            ax, ay = p[..., 0] * iz, p[..., 1] * iz
            e = np.stack([ax - self.xn[..., 0], ay - self.xn[..., 1]], 2)
            r2 = np.where(p[..., 2] > 0, e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1], np.nan)
            act = self.rows & (r2 < self.w[:, 4, None])
        return e, q, iz, ax, ay, r2, act

    def cost(self, R, t, X):
        """(truncated cost, active rows [V, N])"""
        _, _, _, _, _, r2, act = self.residuals(R, t, X)
        term = np.where(act, r2, self.miss[:, None])
        return float(term[self.rows].sum()), act


def jac_cam(q, iz, ax, ay):
    """de / d(w, dt) [..., 2, 6]: dp = e_k x q for the rotation about e_k, e_k for dt_k"""
    z = np.zeros_like(iz)
    r0 = [(0.0 - ax * q[..., 1]) * iz, (q[..., 2] - ax * (-q[..., 0])) * iz, ((-q[..., 1]) - ax * 0.0) * iz, iz, z, (0.0 - ax) * iz]
    r1 = [((-q[..., 2]) - ay * q[..., 1]) * iz, (0.0 - ay * (-q[..., 0])) * iz, (q[..., 0] - ay * 0.0) * iz, z, iz, (0.0 - ay) * iz]
    return np.stack([np.stack(r0, -1), np.stack(r1, -1)], -2)


def jac_pt(R, iz, ax, ay):
    """de / dX [V, N, 2, 3]: dp = R e_k"""
    r0 = (R[:, None, 0, :] - ax[..., None] * R[:, None, 2, :]) * iz[..., None]
    r1 = (R[:, None, 1, :] - ay[..., None] * R[:, None, 2, :]) * iz[..., None]
    return np.stack([r0, r1], -2)


def sym3(v):
    """[n, 3, 3] of the upper triangles v [n, 6]"""
    return np.stack([np.stack([v[:, 0], v[:, 1], v[:, 2]], 1), np.stack([v[:, 1], v[:, 3], v[:, 4]], 1),
                     np.stack([v[:, 2], v[:, 4], v[:, 5]], 1)], 1)


def vi_jpt(vi, Jp):
    """A = Vi Jp^T [n, 3, 2] of Vi's upper triangle vi [n, 6] and Jp [n, 2, 3]"""
    rows = []
    for c, (i0, i1, i2) in enumerate(((0, 1, 2), (1, 3, 4), (2, 4, 5))):
        rows.append(np.stack([(vi[:, i0] * Jp[:, r, 0] + vi[:, i1] * Jp[:, r, 1]) + vi[:, i2] * Jp[:, r, 2] for r in range(2)], 1))
    return np.stack(rows, 1)


def build(P, R, t, X, lam):
    """The normal equations of the state at lam.  Returns a dict: cost, act [V, N], adj [N] (points adjusted), vi [N, 6], gj [N, 3],
    S [6V, 6V] (symmetric, unit rows in place), rhs [6V], free [6V], Jc [V, N, 2, 6], Jp [V, N, 2, 3], e."""
    V, N = P.V, P.N
    e, q, iz, ax, ay, r2, act = P.residuals(R, t, X)
    cost = float(np.where(act, r2, P.miss[:, None])[P.rows].sum())
    with np.errstate(all="ignore"):
        Jc, Jp = jac_cam(q, iz, ax, ay), jac_pt(R, iz, ax, ay)
        Vj, gj = np.zeros((N, 6)), np.zeros((N, 3))
        for i in range(V):  # in view order, as a thread adds them
            a = act[i]
            J = Jp[i, a]
            for k, (c, d) in enumerate(TRI3):
                Vj[a, k] = Vj[a, k] + (J[:, 0, c] * J[:, 0, d] + J[:, 1, c] * J[:, 1, d])
            for c in range(3):
                gj[a, c] = gj[a, c] + (J[:, 0, c] * e[i, a, 0] + J[:, 1, c] * e[i, a, 1])
        na = act.sum(axis=0)
        d0, d1, d2 = Vj[:, 0] + lam * Vj[:, 0], Vj[:, 3] + lam * Vj[:, 3], Vj[:, 5] + lam * Vj[:, 5]
        piv = PIVOT_REL * np.maximum(np.maximum(d0, d1), d2)
        l00 = np.sqrt(d0)
        l10, l20 = Vj[:, 1] / l00, Vj[:, 2] / l00
        p1 = d1 - l10 * l10
        l11 = np.sqrt(p1)
        l21 = (Vj[:, 4] - l20 * l10) / l11
        p2 = (d2 - l20 * l20) - l21 * l21
        l22 = np.sqrt(p2)
        adj = P.inc & (na >= 2) & (d0 > piv) & (p1 > piv) & (p2 > piv)
        a, c, f = 1.0 / l00, 1.0 / l11, 1.0 / l22
        b, g = (0.0 - (l10 * a)) * c, (0.0 - (l21 * c)) * f
        d = (0.0 - (l20 * a + l21 * b)) * f
        vi = np.stack([(a * a + b * b) + d * d, b * c + d * g, d * f, c * c + g * g, g * f, f * f], 1)
    n6 = 6 * V
    S, rhs, udiag = np.zeros((n6, n6)), np.zeros(n6), np.zeros(n6)
    use = act & adj[None]
    A = [None] * V
    for i in range(V):
        r = use[i]
        J, Pi = Jc[i, r], Jp[i, r]
        A[i] = vi_jpt(vi[r], Pi)
        M = np.stack([np.stack([(Pi[:, a_, 0] * A[i][:, 0, s] + Pi[:, a_, 1] * A[i][:, 1, s]) + Pi[:, a_, 2] * A[i][:, 2, s]
                                for s in range(2)], 1) for a_ in range(2)], 1)
        h = np.stack([e[i, r, a_] - ((A[i][:, 0, a_] * gj[r, 0] + A[i][:, 1, a_] * gj[r, 1]) + A[i][:, 2, a_] * gj[r, 2]) for a_ in range(2)], 1)
        D = J - (M[:, :, 0, None] * J[:, None, 0, :] + M[:, :, 1, None] * J[:, None, 1, :])
        blk = (J[:, 0, :, None] * D[:, 0, None, :] + J[:, 1, :, None] * D[:, 1, None, :]).sum(axis=0)
        U = (J[:, 0] * J[:, 0] + J[:, 1] * J[:, 1]).sum(axis=0)
        gr = (J[:, 0] * h[:, 0, None] + J[:, 1] * h[:, 1, None]).sum(axis=0)
        s = slice(6 * i, 6 * i + 6)
        S[s, s] = np.tril(blk) + np.tril(blk, -1).T + np.diag(lam * U)
        udiag[s], rhs[s] = U, 0.0 - gr
    for i in range(V):
        for k in range(i + 1, V):
            r = use[i] & use[k]
            Ji, Jk, Pk = Jc[i, r], Jc[k, r], Jp[k, r]
            Ai = vi_jpt(vi[r], Jp[i, r])
            M = np.stack([np.stack([(Pk[:, a_, 0] * Ai[:, 0, s] + Pk[:, a_, 1] * Ai[:, 1, s]) + Pk[:, a_, 2] * Ai[:, 2, s]
                                    for s in range(2)], 1) for a_ in range(2)], 1)
            Z = 0.0 - (M[:, :, 0, None] * Ji[:, None, 0, :] + M[:, :, 1, None] * Ji[:, None, 1, :])
            blk = (Jk[:, 0, :, None] * Z[:, 0, None, :] + Jk[:, 1, :, None] * Z[:, 1, None, :]).sum(axis=0)
            S[6 * k:6 * k + 6, 6 * i:6 * i + 6] = blk
            S[6 * i:6 * i + 6, 6 * k:6 * k + 6] = blk.T
    free = ~P.hold & (udiag > 0)
    fixed = ~free
    S[fixed, :] = 0.0
    S[:, fixed] = 0.0
    S[fixed, fixed] = 1.0
    rhs[fixed] = 0.0
    return dict(cost=cost, act=act, adj=adj, use=use, vi=vi, gj=gj, S=S, rhs=rhs, free=free, Jc=Jc, Jp=Jp, e=e,
                nres=int(use.sum()))


def solve(S, rhs, free):
    """dc of S dc = rhs by Cholesky (the lower triangle), or None when a pivot of a free row is not above PIVOT_REL x the largest
    free diagonal entry; substitution in the device's order: forward with k ascending, backward with k descending"""
    n = len(rhs)
    A = np.array(S, dtype=np.float64)
    big = A.diagonal()[free].max() if free.any() else -math.inf
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j]
        if free[j] and not d > PIVOT_REL * big:
            return None
        L[j, j] = math.sqrt(d)
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        for c in range(j + 1, n):
            A[c:, c] = A[c:, c] - L[c:, j] * L[c, j]
    y = np.zeros(n)
    for i in range(n):
        s = rhs[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s / L[i, i]
    d = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(n - 1, i, -1):
            s = s - L[k, i] * d[k]
        d[i] = s / L[i, i]
    return d


def back_substitute(P, nb, dc):
    """dX [N, 3] of the camera step dc: Vi_j (-g_j - sum_i W_ij^T dc_i), zero for the points that are not adjusted"""
    w = np.zeros((P.N, 3))
    for i in range(P.V):
        r = nb["use"][i]
        J, Pi, d = nb["Jc"][i, r], nb["Jp"][i, r], dc[6 * i:6 * i + 6]
        u = ((J[:, :, 0] * d[0] + J[:, :, 1] * d[1]) + (J[:, :, 2] * d[2] + J[:, :, 3] * d[3])) + (J[:, :, 4] * d[4] + J[:, :, 5] * d[5])
        w[r] = w[r] + (Pi[:, 0, :] * u[:, 0, None] + Pi[:, 1, :] * u[:, 1, None])
    vi, b = nb["vi"], (0.0 - nb["gj"]) - w
    with np.errstate(all="ignore"):
        dX = np.stack([(vi[:, 0] * b[:, 0] + vi[:, 1] * b[:, 1]) + vi[:, 2] * b[:, 2], (vi[:, 1] * b[:, 0] + vi[:, 3] * b[:, 1]) + vi[:, 4] * b[:, 2],
                       (vi[:, 2] * b[:, 0] + vi[:, 4] * b[:, 1]) + vi[:, 5] * b[:, 2]], 1)
    return np.where(nb["adj"][:, None], dX, 0.0)


def move(R, t, X, dc, dX, adj):
    """the state after the step; a zero delta keeps the bits"""
    Rn, tn = R.copy(), t.copy()
    for i in range(len(R)):
        d = dc[6 * i:6 * i + 6]
        if d[:3].any():
            Rn[i] = rodrigues(d[:3]) @ R[i]
        tn[i] = np.where(d[3:] == 0.0, t[i], t[i] + d[3:])
    Xn = X.copy()
    Xn[adj] = X[adj] + dX[adj]
    return Rn, tn, Xn


def schur_step(P, R, t, X, lam):
    """(dc [6V], dX [N, 3], the normal equations) of one step at lam, or (None, None, nb) when S has a failed pivot"""
    nb = build(P, R, t, X, lam)
    dc = solve(nb["S"], nb["rhs"], nb["free"])
    return (None, None, nb) if dc is None else (dc, back_substitute(P, nb, dc), nb)


def dense_step(P, R, t, X, lam):
    """The same step from the full damped system (H + lam diag H) delta = -g over the camera parameters and the adjusted points,
    solved densely - what the Schur form must reproduce.  Returns (dc [6V], dX [N, 3])."""
    nb = build(P, R, t, X, lam)
    idx = np.nonzero(nb["adj"])[0]
    col = {j: 6 * P.V + 3 * k for k, j in enumerate(idx)}
    rows, res = [], []
    for i in range(P.V):
        for j in np.nonzero(nb["use"][i])[0]:
            for r in range(2):
                row = np.zeros(6 * P.V + 3 * len(idx))
                row[6 * i:6 * i + 6] = nb["Jc"][i, j, r] * nb["free"][6 * i:6 * i + 6]
                row[col[j]:col[j] + 3] = nb["Jp"][i, j, r]
                rows.append(row)
                res.append(nb["e"][i, j, r])
    J, e = np.array(rows), np.array(res)
    H, g = J.T @ J, J.T @ e
    H[np.diag_indices_from(H)] += lam * H.diagonal()
    fixed = np.nonzero(~nb["free"])[0]
    H[fixed, fixed] = 1.0
    d = np.linalg.solve(H, -g)
    dX = np.zeros((P.N, 3))
    dX[idx] = d[6 * P.V:].reshape(-1, 3)
    return d[:6 * P.V], dX


def adjust(X, kpts, K, R, t, thr, max_steps=25, hold=None, count=None, valid=True, trace=None):
    """roma_amd.bundle_adjust for one problem (for a comparison with the device kpts must hold what it reads: f32 values).  X [N, 3], kpts [V, N, 2], K [V, 3, 3] or
    None, R [V, 3, 3], t [V, 3], hold [V, 6] bool (None: default_hold).  Returns a dict: points, R, t, mask [V, N], info =
    (accepted steps, cost evaluations, active rows at the end, points adjusted, free camera parameters, problem fitted),
    cost0, cost.  trace: a list that receives (lambda, |step|, trial cost - current cost) of every cost evaluation."""
    X, R, t = np.array(X, dtype=np.float64), np.array(R, dtype=np.float64), np.array(t, dtype=np.float64).reshape(-1, 3)
    V, N = np.asarray(kpts).shape[:2]
    hold = default_hold(t) if hold is None else hold
    out = dict(points=X, R=R, t=t, mask=np.zeros((V, N), dtype=bool), info=(0, 0, 0, 0, 0, 0), cost0=math.nan, cost=math.nan)
    if not valid or not (np.isfinite(R).all() and np.isfinite(t).all()):
        return out
    P = Problem(X, kpts, K, hold, thr, count)
    X0, R0, t0 = X, R, t
    lam, steps, evals, tr = LAMBDA0, 0, 0, 0
    cur = cost0 = math.nan
    fitted, act = False, None
    while True:
        nb = build(P, R, t, X, lam)
        nadj, nfree = int(nb["adj"].sum()), int(nb["free"].sum())
        can = nfree + 3 * nadj > 0 and 2 * nb["nres"] >= nfree + 3 * nadj
        if evals == 0:
            cur = cost0 = nb["cost"]
            act, evals, fitted = nb["act"], 1, can
        if not can or steps >= max_steps:
            break
        dc = solve(nb["S"], nb["rhs"], nb["free"])
        if dc is None:
            break
        dX = back_substitute(P, nb, dc)
        length = math.sqrt(float(dc @ dc) + float(((dX[:, 0] * dX[:, 0] + dX[:, 1] * dX[:, 1]) + dX[:, 2] * dX[:, 2])[nb["adj"]].sum()))
        if length < STEP_TOL:
            break
        Rn, tn, Xn = move(R, t, X, dc, dX, nb["adj"])
        c, a = P.cost(Rn, tn, Xn)
        evals += 1
        if trace is not None:
            trace.append((lam, length, c - cur))
        if c < cur:
            R, t, X, cur, act = Rn, tn, Xn, c, a
            lam, tr, steps = max(lam / 10.0, LAMBDA_MIN), 0, steps + 1
            if steps >= max_steps:
                break
        else:
            lam, tr = lam * 10.0, tr + 1
            if tr > RETRIES:
                break
    out.update(info=(steps, evals, int(act.sum()), nadj, nfree, int(fitted)), cost0=cost0, cost=cur)
    if fitted:
        out.update(mask=act)
    if steps:
        out.update(points=np.where(P.inc[:, None], X, X0), R=R, t=t)
    return out
