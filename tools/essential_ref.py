"""numpy float64 restatement of the device essential-matrix RANSAC and recoverPose (roma_amd/csrc/essential.hip,
`roma_amd.find_essential` / `recover_pose` / `estimate_pose`): the oracle of tests/test_gpu_essential.py, as
tools/geometry_ref.py is for H and F (whose round loop - sampling stream, selection, iteration count and stop - and
Gauss-Jordan this file imports).

Same algorithm step by step: normalisation x_n = ((x - cx) / fx, (y - cy) / fy) (identity without a camera matrix), threshold
/ ((fx + fy) / 2); hypotheses in rounds of ROUND per pair drawn by the same counter-based generator at S = 5; Nister's
five-point solver with the same schedule, vectorised over samples (null space by Gauss-Jordan, orthonormalised by modified
Gram-Schmidt into the basis X, Y, Z, W;
the ten cubic constraints in Nister's column order; Gauss-Jordan on their ten leading columns; det of the 3 x 3 polynomial
matrix; Sturm chain scaled to unit maximum at each step; BISECT bisection steps per root from Fujiwara's bound, then NEWTON polishing
steps on the polynomial; x, y from the cross product of the two rows of B(z) with the largest last component; unit norm, largest-magnitude entry positive); the Sampson test; the same selection (largest
count, ties to the lowest (h, root)) and stopping rule; recoverPose with the same one-sided Jacobi SVD, OpenCV's fix-up and the
same linear triangulation (point on the ray of camera 0, two equations of camera 1).  Differences by design: the device
scores in f32 (here f64, so masks can differ at points whose error lies at the threshold), and sums in its own order, so
Sturm bisection can end one rounding step apart.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_ref as gr  # noqa: E402

MAX_ROOTS = 10
BISECT = 64
NEWTON = 3
NEWTON_REACH = 1e-3  # relative size of a Newton step that is still taken
GN_STEPS = 3
GN_REACH = 1e-2
E_PIVOT_EPS = 1e-10
SVD_SWEEPS = 20
SVD_TOL = 4 * np.finfo(np.float64).eps

# Nister's column order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
_MONO = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
_VAR = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]  # a linear polynomial: coefficients of x, y, z, 1
_TRIPLE = np.zeros((64, 20))  # [a b c] -> monomial of var_a var_b var_c
for _a in range(4):
    for _b in range(4):
        for _c in range(4):
            _e = tuple(_VAR[_a][k] + _VAR[_b][k] + _VAR[_c][k] for k in range(3))
            _TRIPLE[_a * 16 + _b * 4 + _c, _MONO.index(_e)] = 1.0


def _triple(p, q, r):
    """product of three batches of linear polynomials [M, 4] -> [M, 20]"""
    return np.einsum("ma,mb,mc->mabc", p, q, r).reshape(len(p), 64) @ _TRIPLE


def null_basis(x0, x1):
    """unit-norm basis X, Y, Z, W [M, 9, 4] (entry k of E: coefficients of x, y, z, 1) of the 5 x 9 system, and ok [M]"""
    x, y, u, v = x0[..., 0], x0[..., 1], x1[..., 0], x1[..., 1]
    a = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], axis=-1)
    r, ok = gr.gauss_jordan(a)
    m = len(x0)
    basis = np.zeros((m, 9, 4))
    for f in range(4):  # modified Gram-Schmidt in the order X, Y, Z, W
        vec = np.zeros((m, 9))
        vec[:, :5] = -r[:, :, 5 + f]
        vec[:, 5 + f] = 1.0
        for g in range(f):
            vec = vec - (vec * basis[:, :, g]).sum(axis=1)[:, None] * basis[:, :, g]
        basis[:, :, f] = vec / np.sqrt((vec * vec).sum(axis=1))[:, None]
    return basis, ok


def constraints(basis):
    """the 10 x 20 cubic constraints [M, 10, 20]: rows 3 i + j = 2 (E E^T E)_ij - tr(E E^T) E_ij, row 9 = det E"""
    P = lambda i, j: basis[:, 3 * i + j]  # noqa: E731
    m = len(basis)
    C = np.zeros((m, 10, 20))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                for l in range(3):
                    C[:, 3 * i + j] += 2.0 * _triple(P(i, l), P(k, l), P(k, j)) - _triple(P(k, l), P(k, l), P(i, j))
    for q, (a, b, c) in enumerate(((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0))):
        C[:, 9] += (1.0 if q < 3 else -1.0) * _triple(P(0, a), P(1, b), P(2, c))
    return C


def gauss_jordan10(C):
    """Gauss-Jordan with partial pivoting (first maximum) on columns 0 .. 9 of [M, 10, 20]: (reduced, ok)"""
    a = np.array(C, dtype=np.float64)
    m = len(a)
    ar = np.arange(m)
    ok = np.ones(m, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(10):
            col = np.abs(a[:, k:, k])
            p = k + np.argmax(col, axis=1)
            ok &= col[ar, p - k] > E_PIVOT_EPS
            rk, rp = a[ar, k].copy(), a[ar, p].copy()
            a[ar, k], a[ar, p] = rp, rk
            a[:, k, :] = a[:, k, :] * (1.0 / a[:, k, k])[:, None]
            for r in range(10):
                if r != k:
                    a[:, r, :] = a[:, r, :] - a[:, r, k].copy()[:, None] * a[:, k, :]
    return a, ok


def nister_rows(red):
    """B(z) rows <e> - z <f>, <g> - z <h>, <i> - z <j>: (bx [M, 3, 4], by [M, 3, 4], b1 [M, 3, 5]), ascending in z"""
    e, f = red[:, 4::2, 10:], red[:, 5::2, 10:]
    bx = np.stack([e[..., 2], e[..., 1] - f[..., 2], e[..., 0] - f[..., 1], -f[..., 0]], axis=-1)
    by = np.stack([e[..., 5], e[..., 4] - f[..., 5], e[..., 3] - f[..., 4], -f[..., 3]], axis=-1)
    b1 = np.stack([e[..., 9], e[..., 8] - f[..., 9], e[..., 7] - f[..., 8], e[..., 6] - f[..., 7], -f[..., 6]], axis=-1)
    return bx, by, b1


def _pmul(a, b):
    out = np.zeros(a.shape[:-1] + (a.shape[-1] + b.shape[-1] - 1,))
    for i in range(a.shape[-1]):
        for j in range(b.shape[-1]):
            out[..., i + j] += a[..., i] * b[..., j]
    return out


def _scale_max(p):
    with np.errstate(all="ignore"):
        return p * (1.0 / np.abs(p).max(axis=-1))[:, None]


def _horner(c, t):
    v = c[..., -1]
    for i in range(c.shape[-1] - 2, -1, -1):
        v = v * t + c[..., i]
    return v


def sturm_chain(p0):
    """[p0, p0', -rem, ...] with the generic degree drop, each scaled to unit maximum"""
    p0 = _scale_max(p0)
    p1 = _scale_max(p0[:, 1:] * np.arange(1, 11)[None])
    chain = [p0, p1]
    a, b = p0, p1
    with np.errstate(all="ignore"):
        while b.shape[1] > 1:
            n = a.shape[1]
            q1 = a[:, n - 1] / b[:, n - 2]
            q0 = (a[:, n - 2] - q1 * b[:, n - 3]) / b[:, n - 2]
            r = np.zeros((len(a), n - 2))
            r[:, 0] = -(a[:, 0] - q0 * b[:, 0])
            for i in range(1, n - 2):
                r[:, i] = -((a[:, i] - q1 * b[:, i - 1]) - q0 * b[:, i])
            r = _scale_max(r)
            chain.append(r)
            a, b = b, r
    return chain


def _changes(vals):
    """sign changes along the chain axis (list of arrays), zeros skipped"""
    c = np.zeros(vals[0].shape, dtype=np.int64)
    last = np.zeros(vals[0].shape)
    for v in vals:
        nz = v != 0
        c += (nz & (last != 0) & ((v < 0) != (last < 0))).astype(np.int64)
        last = np.where(nz, v, last)
    return c


def _cofactor(E):
    e = E.reshape(E.shape[:-2] + (9,))
    c = [e[..., 4] * e[..., 8] - e[..., 5] * e[..., 7], e[..., 5] * e[..., 6] - e[..., 3] * e[..., 8],
         e[..., 3] * e[..., 7] - e[..., 4] * e[..., 6], e[..., 2] * e[..., 7] - e[..., 1] * e[..., 8],
         e[..., 0] * e[..., 8] - e[..., 2] * e[..., 6], e[..., 1] * e[..., 6] - e[..., 0] * e[..., 7],
         e[..., 1] * e[..., 5] - e[..., 2] * e[..., 4], e[..., 2] * e[..., 3] - e[..., 0] * e[..., 5],
         e[..., 0] * e[..., 4] - e[..., 1] * e[..., 3]]
    return np.stack(c, axis=-1).reshape(E.shape)


def refine(basis, x, y, z):
    """GN_STEPS Gauss-Newton steps of (x, y, z) [M, R] on the ten cubic constraints of E = x X + y Y + z Z + W themselves (not
    on the eliminated polynomial, whose roots carry the elimination's rounding); a step longer than GN_REACH (1 + max |x, y, z|)
    or not finite is not taken.  The 3 x 3 normal equations are solved by Cramer's rule."""
    m = len(basis)
    Bm = basis.reshape(m, 1, 3, 3, 4)
    D = [Bm[..., k] for k in range(3)]
    for _ in range(GN_STEPS):
        E = ((x[..., None, None] * D[0] + y[..., None, None] * D[1]) + z[..., None, None] * D[2]) + Bm[..., 3]
        Et = np.swapaxes(E, -1, -2)
        EEt = E @ Et
        tr = np.trace(EEt, axis1=-2, axis2=-1)[..., None, None]
        r = np.concatenate([(2.0 * (EEt @ E) - tr * E).reshape(E.shape[:-2] + (9,)), np.linalg.det(E)[..., None]], axis=-1)
        cof = _cofactor(E)
        J = []
        for Dk in D:
            ip = (Dk * E).sum(axis=(-2, -1))[..., None, None]
            d1 = 2.0 * ((Dk @ Et @ E + E @ np.swapaxes(Dk, -1, -2) @ E) + EEt @ Dk) - 2.0 * ip * E - tr * Dk
            J.append(np.concatenate([d1.reshape(E.shape[:-2] + (9,)), (cof * Dk).sum(axis=(-2, -1))[..., None]], axis=-1))
        A = np.stack([np.stack([(J[i] * J[j]).sum(-1) for j in range(3)], -1) for i in range(3)], -2)  # [M, R, 3, 3]
        g = np.stack([(J[i] * r).sum(-1) for i in range(3)], -1)
        det = np.linalg.det(A)
        step = []
        for k in range(3):
            Ak = A.copy()
            Ak[..., :, k] = g
            step.append(-np.linalg.det(Ak) / det)
        big = 1.0 + np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))
        take = np.isfinite(step[0]) & np.isfinite(step[1]) & np.isfinite(step[2])
        take &= np.maximum(np.maximum(np.abs(step[0]), np.abs(step[1])), np.abs(step[2])) <= GN_REACH * big
        x, y, z = np.where(take, x + step[0], x), np.where(take, y + step[1], y), np.where(take, z + step[2], z)
    return x, y, z


def five_point(x0, x1):
    """Nister's five-point solver on samples [M, 5, 2]: (E [M, 10, 3, 3] unit norm, largest-magnitude entry positive, zeros
    beyond n; n [M]) in ascending order of z"""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    with np.errstate(all="ignore"):
        basis, ok = null_basis(x0, x1)
    return solve_basis(basis, ok)


def solve_basis(basis, ok):
    """the solver from a unit-norm basis X, Y, Z, W [M, 9, 4] on (five_point: a sample's null space; essential_magsac_ref: the
    least-squares null space of more rows): the real E = x X + y Y + z Z + W that satisfy the cubic constraints, as five_point
    returns them"""
    m = len(basis)
    ok = np.array(ok, dtype=bool)
    with np.errstate(all="ignore"):
        red, ok2 = gauss_jordan10(constraints(basis))
        ok &= ok2
        bx, by, b1 = nister_rows(red)
        u = _pmul(by[:, 1], b1[:, 2]) - _pmul(b1[:, 1], by[:, 2])
        v = _pmul(bx[:, 1], b1[:, 2]) - _pmul(b1[:, 1], bx[:, 2])
        w = _pmul(bx[:, 1], by[:, 2]) - _pmul(by[:, 1], bx[:, 2])
        p0 = (_pmul(bx[:, 0], u) - _pmul(by[:, 0], v)) + _pmul(b1[:, 0], w)
        chain = sturm_chain(p0)
        fin = np.all([np.isfinite(c).all(axis=1) for c in chain], axis=0)
        lead = np.stack([c[:, -1] for c in chain], axis=1)  # [M, 11], degree 10 - j
        fin &= (lead != 0).all(axis=1)
        vpos = _changes(list(lead.T))
        vneg = _changes(list((lead * np.array([(-1.0) ** (10 - j) for j in range(11)])[None]).T))
        c = chain[0]
        bound = np.zeros(m)
        for i in range(1, 11):  # Fujiwara's bound of the roots: 2 max_i |a_{10-i} / a_10|^(1/i)
            bound = np.maximum(bound, np.power(np.abs(c[:, 10 - i] / c[:, 10]), 1.0 / i))
        bound = 2.0 * bound
        fin &= np.isfinite(bound)
        nroots = np.where(fin & ok, np.clip(vneg - vpos, 0, MAX_ROOTS), 0)
        k = np.arange(MAX_ROOTS)[None, :]
        lo, hi = np.repeat(-bound[:, None], MAX_ROOTS, 1), np.repeat(bound[:, None], MAX_ROOTS, 1)
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            cnt = vneg[:, None] - _changes([_horner(c[:, None, :], mid) for c in chain])
            up = cnt >= k + 1
            lo, hi = np.where(up, lo, mid), np.where(up, mid, hi)
        z = 0.5 * (lo + hi)
        dp = chain[0][:, 1:] * np.arange(1, 11)[None]
        for _ in range(NEWTON):  # polish on p0; a step that leaves the bisection bracket's neighbourhood is not taken
            z1 = z - _horner(chain[0][:, None, :], z) / _horner(dp[:, None, :], z)
            z = np.where(np.isfinite(z1) & (np.abs(z1 - z) <= NEWTON_REACH * (1.0 + np.abs(z))), z1, z)
        ev = lambda c: _horner(c[:, None, :], z)  # noqa: E731
        rows = [(ev(bx[:, r]), ev(by[:, r]), ev(b1[:, r])) for r in range(3)]
        c0, c1, c2 = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z)
        for a, b in ((0, 1), (0, 2), (1, 2)):  # the cross product of two rows with the largest |w| (first on ties)
            (kx, ky, k1), (lx, ly, l1) = rows[a], rows[b]
            d0, d1, d2 = ky * l1 - k1 * ly, k1 * lx - kx * l1, kx * ly - ky * lx
            take = np.abs(d2) > np.abs(c2)
            c0, c1, c2 = np.where(take, d0, c0), np.where(take, d1, c1), np.where(take, d2, c2)
        x, y = c0 / c2, c1 / c2
        x, y, z = refine(basis, x, y, z)
        E = ((x[..., None] * basis[:, None, :, 0] + y[..., None] * basis[:, None, :, 1]) + z[..., None] * basis[:, None, :, 2]) \
            + basis[:, None, :, 3]  # [M, 10, 9]
        E = E * (1.0 / np.sqrt((E * E).sum(axis=-1)))[..., None]
        big = np.argmax(np.abs(E), axis=-1)
        sg = np.where(np.take_along_axis(E, big[..., None], -1)[..., 0] < 0, -1.0, 1.0)
        E = E * sg[..., None]
        valid = (k < nroots[:, None]) & np.isfinite(E).all(axis=-1)
    out = np.zeros((m, MAX_ROOTS, 9))
    n = valid.sum(axis=1)
    for i in np.nonzero(n)[0]:
        out[i, :n[i]] = E[i, valid[i]]
    return out.reshape(m, MAX_ROOTS, 3, 3), n


def inliers(E, x0, x1, t2):
    """Sampson test of models E [K, 3, 3] on normalised points [n, 2] (NaN never passes): [K, n]"""
    m = E.reshape(-1, 9)[:, :, None]
    x, y, u, v = x0[None, :, 0], x0[None, :, 1], x1[None, :, 0], x1[None, :, 1]
    with np.errstate(invalid="ignore"):
        lx, ly, lz = m[:, 0] * x + m[:, 1] * y + m[:, 2], m[:, 3] * x + m[:, 4] * y + m[:, 5], m[:, 6] * x + m[:, 7] * y + m[:, 8]
        d = u * lx + v * ly + lz
        kx, ky = m[:, 0] * u + m[:, 3] * v + m[:, 6], m[:, 1] * u + m[:, 4] * v + m[:, 7]
        return d * d < t2 * ((lx * lx + ly * ly) + (kx * kx + ky * ky))


def _normalise(p, K):
    if K is None:
        return np.array(p, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]], axis=1)


def ransac(pa, pb, thr, prob, max_iters, seed, K=None):
    """One pair of findEssentialMat.  pa, pb [n, 2] (rows of the pair only; what the device reads, i.e. f32-rounded).
    Returns a dict: E [3, 3] (or zeros), mask [n], ok, rounds, best_h, best_root, best."""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    n = len(pa)
    out = dict(E=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), ok=False, rounds=0, best_h=-1, best_root=-1, best=-1)
    thr_n = float(thr) if K is None else float(thr) / ((K[0, 0] + K[1, 1]) * 0.5)
    fin = np.isfinite(pa).all(axis=1) & np.isfinite(pb).all(axis=1)
    if n < 5 or fin.sum() < 5:
        return out
    with np.errstate(invalid="ignore"):
        xa, xb = _normalise(pa, K), _normalise(pb, K)
    t2 = thr_n * thr_n
    _, best, cur, best_h, best_root, rounds = gr.round_loop(n, 5, MAX_ROOTS, fin, seed, prob, max_iters,
                                                            lambda idx: five_point(xa[idx], xb[idx]),
                                                            lambda M: (inliers(M, xa, xb, t2).sum(axis=1),) * 2)
    out.update(rounds=rounds, best_h=best_h, best_root=best_root)
    if best <= 0:
        return out
    out.update(E=cur, mask=inliers(cur[None], xa, xb, t2)[0], ok=True, best=best)
    return out


def find_essential(pa, pb, camera_matrix=None, prob=0.999, threshold=1.0, max_iters=1000, seed=0):
    """cv2.findEssentialMat restated: (E [3, 3] or None, mask [n] or None)"""
    r = ransac(pa, pb, threshold, prob, max_iters, seed, camera_matrix)
    return (r["E"], r["mask"]) if r["ok"] else (None, None)


# ---------------------------------------------------------------------------------------------------- recoverPose
_W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def svd3(E):
    """the device's SVD of a 3 x 3: one-sided Jacobi on the columns, descending singular values, u3 = u1 x u2 (v3 signed to
    match).  Returns (U, s, Vt) or None when the rank is below 2 or a value is not finite."""
    A = np.array(E, dtype=np.float64).copy()
    V = np.eye(3)
    if not np.isfinite(A).all():
        return None
    for _ in range(SVD_SWEEPS):
        rot = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al, be, ga = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
            if abs(ga) > SVD_TOL * math.sqrt(al * be):
                z = (be - al) / (2 * ga)
                tn = math.copysign(1.0, z) / (abs(z) + math.sqrt(1 + z * z))
                c = 1 / math.sqrt(1 + tn * tn)
                s = c * tn
                A[:, [p, q]] = np.stack([c * A[:, p] - s * A[:, q], s * A[:, p] + c * A[:, q]], 1)
                V[:, [p, q]] = np.stack([c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]], 1)
                rot = True
        if not rot:
            break
    sg = np.linalg.norm(A, axis=0)
    for p in (0, 1, 0):
        if sg[p + 1] > sg[p]:
            sg[[p, p + 1]], A[:, [p, p + 1]], V[:, [p, p + 1]] = sg[[p + 1, p]], A[:, [p + 1, p]], V[:, [p + 1, p]]
    if not sg[1] > 0:
        return None
    U = np.zeros((3, 3))
    U[:, 0], U[:, 1] = A[:, 0] / sg[0], A[:, 1] / sg[1]
    U[:, 2] = np.cross(U[:, 0], U[:, 1])
    if A[:, 2] @ U[:, 2] < 0:
        V[:, 2] = -V[:, 2]
    return U, sg, V.T


def decompose(E):
    """the four candidates [(R1, t), (R2, t), (R1, -t), (R2, -t)] in OpenCV's order, or None"""
    r = svd3(E)
    if r is None:
        return None
    U, _, Vt = r
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    R1, R2, t = U @ _W @ Vt, U @ _W.T @ Vt, U[:, 2]
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def cheirality(R, t, x0, x1, dist):
    """the device's linear triangulation (X = (lam x0, w), least squares in camera 1) and OpenCV's rule: [n] bool"""
    r = np.c_[x0, np.ones(len(x0))] @ R.T
    u, v = x1[:, 0], x1[:, 1]
    a1, b1 = u * r[:, 2] - r[:, 0], u * t[2] - t[0]
    a2, b2 = v * r[:, 2] - r[:, 1], v * t[2] - t[1]
    p, q, s = a1 * a1 + a2 * a2, a1 * b1 + a2 * b2, b1 * b1 + b2 * b2
    hd = (p - s) * 0.5
    mu = (p + s) * 0.5 - np.sqrt(hd * hd + q * q)
    lam = np.where(p >= s, q, mu - s)
    w = np.where(p >= s, mu - p, q)
    with np.errstate(all="ignore"):
        z0, z1 = lam / w, (lam * r[:, 2] + w * t[2]) / w
        return (lam * w > 0) & (z0 < dist) & (z1 > 0) & (z1 < dist)


def recover_pose(E, x0, x1, mask=None, distance_thresh=1e9):
    """cv2.recoverPose restated on normalised points: (n_good, R, t [3, 1], mask_good [n]); (0, None, None, zeros) when E
    cannot be decomposed"""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    n = len(x0)
    cands = decompose(E)
    sel = np.isfinite(x0).all(axis=1) & np.isfinite(x1).all(axis=1)
    if mask is not None:
        sel &= np.asarray(mask, dtype=bool)
    if cands is None:
        return 0, None, None, np.zeros(n, dtype=bool)
    goods = [sel & cheirality(R, t, x0, x1, distance_thresh) for R, t in cands]
    c = int(np.argmax([g.sum() for g in goods]))
    return int(goods[c].sum()), cands[c][0], cands[c][1][:, None].copy(), goods[c]


def estimate_pose(kpts0, kpts1, K0, K1, norm_thresh, conf=0.99999, max_iters=1000, seed=0):
    """romatch/utils/utils.py:30-51 as the device runs it: (R, t [3, 1], mask) or None; mask = RANSAC inliers that pass the
    cheirality test of the chosen candidate.  The normalised points are rounded to f32, as the device's kernels read them."""
    if len(kpts0) < 5:
        return None
    K0inv, K1inv = np.linalg.inv(K0[:2, :2]), np.linalg.inv(K1[:2, :2])
    x0 = (K0inv @ (np.asarray(kpts0, dtype=np.float64) - K0[None, :2, 2]).T).T.astype(np.float32).astype(np.float64)
    x1 = (K1inv @ (np.asarray(kpts1, dtype=np.float64) - K1[None, :2, 2]).T).T.astype(np.float32).astype(np.float64)
    r = ransac(x0, x1, norm_thresh, conf, max_iters, seed)
    if not r["ok"]:
        return None
    n, R, t, good = recover_pose(r["E"], x0, x1, r["mask"])
    if n == 0:
        return None
    return R, t, good
