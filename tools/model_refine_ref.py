"""numpy float64 restatement of the device refinement of homographies and fundamental matrices (roma_amd/csrc/model_refine.hip,
`roma_amd.refine_homography` / `refine_fundamental`, `find_*(..., lm_steps=k)`): the oracle of tests/test_gpu_model_refine.py, as
tools/pose_refine_ref.py is for the pose refinement; the loop of both is tools/lm_ref.py.

A Levenberg-Marquardt fit of the model to the rows inside the threshold, under the hard-truncated loss: the reprojection error
in image B for H (what cv2.findHomography(..., RANSAC) ends with) and the Sampson distance for F (what PoseLib's
estimate_fundamental ends with).  Neither library is a dependency or restated: the algorithm below is its own definition.

Common to both models (one pair; M [3, 3] in pixel coordinates, points [n, 2] pixels, thr in pixels):
  coordinates x^ = (x - c) s with (c_a, s_a, c_b, s_b) of geometry_ref.normalize over the finite rows; the fit runs on
              M^ = T_b M T_a^-1 (H) or T_b^-T M T_a^-1 (F) scaled to unit Frobenius norm; residuals are in pixels
  loop        cost, iteration and stopping rules are lm_ref.fit's, which tools/pose_refine_ref.py shares; thr = inf is plain
              least squares over the finite rows; the active set is that of the model under evaluation, not the RANSAC mask
  output      the model de-normalised and scaled like geometry_ref.ransac's (the input itself when no step was accepted),
              mask = active under the final model, info = (accepted steps, cost evaluations, active rows at the end, pair
              fitted), cost = (start, final) truncated cost in px^2

Homography (MIN_ROWS 4, 8 parameters, two residuals per row):
  p = H^ (x^, y^, 1), e = ((p_x / p_z - u^) / s_b, (p_y / p_z - v^) / s_b): the forward reprojection error in image B
  gauge: the entry of the unit-norm start H^ with the largest magnitude (first maximum, row-major) is held fixed, the other
  eight are updated additively.
Fundamental matrix (MIN_ROWS 7, 7 parameters, one residual per row):
  l = F^ x^_a, k = F^T x^_b, c = x^_b . l, r = c / sqrt(s_b^2 (l_0^2 + l_1^2) + s_a^2 (k_0^2 + k_1^2)): the signed Sampson
  distance in pixels (x_b^T F x_a = x^_b^T F^ x^_a)
  F^ = U diag(1, sigma, 0) V^T with U, V rotations (`svd_rank2`: one-sided Jacobi, as the kernel; u_2 = u_0 x u_1,
  v_2 = v_0 x v_1, so a start that is not rank 2 is projected); parameters (a, b, d): U <- U exp([a]x), V <- V exp([b]x),
  sigma <- sigma + d.  Rank 2 holds at every iterate.
The device sums H, g and the cost in its own fixed order and calls its own sin / cos / sqrt: the two agree to rounding.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_ref as gr  # noqa: E402
import lm_ref  # noqa: E402
from lm_ref import LAMBDA0, LAMBDA_MIN, PIVOT_REL, RETRIES, STEP_TOL, active, solve, truncated  # noqa: E402,F401
from pose_refine_ref import rodrigues  # noqa: E402

HOMOGRAPHY, FUNDAMENTAL = gr.HOMOGRAPHY, gr.FUNDAMENTAL
MIN_ROWS = {HOMOGRAPHY: 4, FUNDAMENTAL: 7}  # rows of a pair, and active rows of an iteration, below which nothing is fitted
NPAR = {HOMOGRAPHY: 8, FUNDAMENTAL: 7}
SVD_SWEEPS = 20
SVD_TOL = 4 * np.finfo(np.float64).eps


def mat3(a, b):
    """a b with the sums in the kernel's order"""
    c = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            c[i, j] = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
    return c


def fro(m):
    m = np.asarray(m).reshape(9)
    s = 0.0
    for k in range(9):
        s = s + m[k] * m[k]
    return math.sqrt(s)


def transforms(model, ca, sa, cb, sb):
    """(L, Rm, Li, Ta): M^ = L M Rm and M = Li M^ Ta"""
    Ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1]])
    Rm = np.array([[1 / sa, 0, ca[0]], [0, 1 / sa, ca[1]], [0, 0, 1]])
    if model == HOMOGRAPHY:
        L = np.array([[sb, 0, -sb * cb[0]], [0, sb, -sb * cb[1]], [0, 0, 1]])
        Li = np.array([[1 / sb, 0, cb[0]], [0, 1 / sb, cb[1]], [0, 0, 1]])
    else:
        L = np.array([[1 / sb, 0, 0], [0, 1 / sb, 0], [cb[0], cb[1], 1]])
        Li = np.array([[sb, 0, 0], [0, sb, 0], [-sb * cb[0], -sb * cb[1], 1]])
    return L, Rm, Li, Ta


def denormalise(model, Mn, ca, sa, cb, sb):
    """the last lines of geometry_ref.ransac"""
    _, _, Li, Ta = transforms(model, ca, sa, cb, sb)
    M = mat3(mat3(Li, Mn), Ta)
    f = fro(M)
    return M / (M[2, 2] if abs(M[2, 2]) >= 1e-12 * f else f)


class Rows:
    """the normalised rows of a pair and its scales"""

    def __init__(self, x, y, u, v, sa, sb):
        self.x, self.y, self.u, self.v, self.sa, self.sb = x, y, u, v, sa, sb


class _Fit:
    """what the two problems below share of lm_ref.fit's policy"""

    @classmethod
    def normal(cls, J, e, a):
        Ja, ea = J[a].reshape(-1, cls.NPAR), e[a].reshape(-1)
        return Ja.T @ Ja, Ja.T @ ea


# ------------------------------------------------------------------------------------------------------------ homography
class HomographyFit(_Fit):
    """state (h [9] row-major, k0 the fixed entry)"""
    MODEL, NPAR, NRES, MIN_ROWS = HOMOGRAPHY, 8, 2, 4

    @staticmethod
    def init(Mn):
        h = np.array(Mn, dtype=np.float64).reshape(9)
        return h, int(np.argmax(np.abs(h)))  # first maximum

    @staticmethod
    def matrix(st):
        return st[0].reshape(3, 3).copy()

    @staticmethod
    def _parts(st, w):
        h = st[0]
        p = [(h[3 * i] * w.x + h[3 * i + 1] * w.y) + h[3 * i + 2] for i in range(3)]
        isb = 1.0 / w.sb
        return p, isb

    @classmethod
    def residuals(cls, st, w):
        """e [n, 2] pixels"""
        with np.errstate(all="ignore"):
            p, isb = cls._parts(st, w)
            return np.stack([(p[0] / p[2] - w.u) * isb, (p[1] / p[2] - w.v) * isb], axis=1)

    @classmethod
    def jacobian(cls, st, w):
        """(e [n, 2], J [n, 2, 8])"""
        with np.errstate(all="ignore"):
            p, isb = cls._parts(st, w)
            e = np.stack([(p[0] / p[2] - w.u) * isb, (p[1] / p[2] - w.v) * isb], axis=1)
            iz = 1.0 / p[2]
            a = iz * isb
            qx, qy = (p[0] * iz) * a, (p[1] * iz) * a
            z = np.zeros_like(w.x)
            c = (w.x * a, w.y * a, a)
            Jx = [c[0], c[1], c[2], z, z, z, -(qx * w.x), -(qx * w.y), -qx]
            Jy = [z, z, z, c[0], c[1], c[2], -(qy * w.x), -(qy * w.y), -qy]
            keep = [k for k in range(9) if k != st[1]]
            J = np.stack([np.stack([Jx[k] for k in keep], axis=1), np.stack([Jy[k] for k in keep], axis=1)], axis=1)
            return e, J

    @staticmethod
    def apply(st, d):
        h = st[0].copy()
        keep = [k for k in range(9) if k != st[1]]
        for j, k in enumerate(keep):
            h[k] = h[k] + d[j]
        return h, st[1]


# ------------------------------------------------------------------------------------------------------------ fundamental
def svd_rank2(F):
    """(U, V, sigma) with F ~ U diag(1, sigma, 0) V^T, U and V rotations: one-sided Jacobi on the columns of F (A V = U S),
    pairs (0, 1), (0, 2), (1, 2) per sweep, singular values sorted descending by the exchanges (0, 1), (1, 2), (0, 1);
    u_2 = u_0 x u_1, v_2 = v_0 x v_1.  None where the second singular value is not positive."""
    a = [np.array(F[:, j], dtype=np.float64) for j in range(3)]  # columns
    v = [np.eye(3)[j].copy() for j in range(3)]
    for _ in range(SVD_SWEEPS):
        rot = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al = be = ga = 0.0
            for k in range(3):
                al += a[p][k] * a[p][k]
                be += a[q][k] * a[q][k]
                ga += a[p][k] * a[q][k]
            if abs(ga) > SVD_TOL * math.sqrt(al * be):
                zz = (be - al) / (2 * ga)
                tn = math.copysign(1.0, zz) / (abs(zz) + math.sqrt(1 + zz * zz))
                c = 1 / math.sqrt(1 + tn * tn)
                s = c * tn
                a[p], a[q] = c * a[p] - s * a[q], s * a[p] + c * a[q]
                v[p], v[q] = c * v[p] - s * v[q], s * v[p] + c * v[q]
                rot = True
        if not rot:
            break
    sg = [math.sqrt((a[j][0] * a[j][0] + a[j][1] * a[j][1]) + a[j][2] * a[j][2]) for j in range(3)]
    for p in (0, 1, 0):
        q = p + 1
        if sg[q] > sg[p]:
            sg[p], sg[q], a[p], a[q], v[p], v[q] = sg[q], sg[p], a[q], a[p], v[q], v[p]
    if not (sg[1] > 0 and math.isfinite(sg[0])):
        return None
    u0, u1 = a[0] / sg[0], a[1] / sg[1]
    U = np.stack([u0, u1, cross(u0, u1)], axis=1)
    V = np.stack([v[0], v[1], cross(v[0], v[1])], axis=1)
    return U, V, sg[1] / sg[0]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def outer(a, b):
    return np.array([[a[i] * b[j] for j in range(3)] for i in range(3)])


class FundamentalFit(_Fit):
    """state (U, V, sigma)"""
    MODEL, NPAR, NRES, MIN_ROWS = FUNDAMENTAL, 7, 1, 7

    @staticmethod
    def init(Mn):
        return svd_rank2(np.asarray(Mn, dtype=np.float64))

    @staticmethod
    def matrix(st):
        U, V, sg = st
        return outer(U[:, 0], V[:, 0]) + sg * outer(U[:, 1], V[:, 1])

    @staticmethod
    def derivatives(st):
        """dF^ by (a0, a1, a2, b0, b1, b2, d) at zero: [7, 3, 3]"""
        U, V, sg = st
        u0, u1, u2, v0, v1, v2 = U[:, 0], U[:, 1], U[:, 2], V[:, 0], V[:, 1], V[:, 2]
        return np.stack([sg * outer(u2, v1), -outer(u2, v0), outer(u1, v0) - sg * outer(u0, v1),
                         sg * outer(u1, v2), -outer(u0, v2), outer(u0, v1) - sg * outer(u1, v0), outer(u1, v1)])

    @staticmethod
    def _parts(F, w):
        l = [(F[i, 0] * w.x + F[i, 1] * w.y) + F[i, 2] for i in range(3)]
        k = [(F[0, j] * w.u + F[1, j] * w.v) + F[2, j] for j in range(2)]
        c = (w.u * l[0] + w.v * l[1]) + l[2]
        return l, k, c

    @classmethod
    def residuals(cls, st, w):
        """r [n, 1] pixels"""
        with np.errstate(all="ignore"):
            l, k, c = cls._parts(cls.matrix(st), w)
            den = (w.sb * w.sb) * (l[0] * l[0] + l[1] * l[1]) + (w.sa * w.sa) * (k[0] * k[0] + k[1] * k[1])
            return (c / np.sqrt(den))[:, None]

    @classmethod
    def jacobian(cls, st, w):
        """(r [n, 1], J [n, 1, 7])"""
        with np.errstate(all="ignore"):
            sa2, sb2 = w.sa * w.sa, w.sb * w.sb
            l, k, c = cls._parts(cls.matrix(st), w)
            den = sb2 * (l[0] * l[0] + l[1] * l[1]) + sa2 * (k[0] * k[0] + k[1] * k[1])
            s = np.sqrt(den)
            r = c / s
            inv_s, inv_den = 1.0 / s, 1.0 / den
            # dF^ of every parameter is a combination of u_i v_j^T, for which dl = u_i al_j, dk = v_j be_i, dc = be_i al_j with
            # al_j = v_j . x^_a, be_i = u_i . x^_b: T(i, j) is dr of u_i v_j^T
            U, V, sg = st
            al = [(V[0, j] * w.x + V[1, j] * w.y) + V[2, j] for j in range(3)]
            be = [(U[0, i] * w.u + U[1, i] * w.v) + U[2, i] for i in range(3)]
            Lu = [(l[0] * U[0, i] + l[1] * U[1, i]) * sb2 for i in range(3)]
            Kv = [(k[0] * V[0, j] + k[1] * V[1, j]) * sa2 for j in range(3)]

            def T(i, j):
                return (be[i] * al[j]) * inv_s - r * ((Lu[i] * al[j] + Kv[j] * be[i]) * inv_den)
            cols = [sg * T(2, 1), -T(2, 0), T(1, 0) - sg * T(0, 1), sg * T(1, 2), -T(0, 2), T(0, 1) - sg * T(1, 0), T(1, 1)]
            return r[:, None], np.stack(cols, axis=1)[:, None, :]

    @staticmethod
    def apply(st, d):
        U, V, sg = st
        return mat3(U, rodrigues(d[0:3])), mat3(V, rodrigues(d[3:6])), sg + d[6]


FITS = {HOMOGRAPHY: HomographyFit, FUNDAMENTAL: FundamentalFit}


# ------------------------------------------------------------------------------------------------------------ the pair
def as_f32(p):
    """points rounded to f32, as the device reads them"""
    return np.asarray(p, dtype=np.float32).astype(np.float64)


def prepare(model, M, pa, pb):
    """the pair as the fit sees it: (rows, M^ of unit norm or None, (ca, sa, cb, sb)).  The points are taken as given: pass
    `as_f32` of them to see what the device, which reads f32, sees."""
    pa, pb = np.asarray(pa, dtype=np.float64).reshape(-1, 2), np.asarray(pb, dtype=np.float64).reshape(-1, 2)
    ca, sa, cb, sb, fin, cnt = gr.normalize(pa, pb)
    if not (cnt > 0 and math.isfinite(sa) and math.isfinite(sb)):
        return None, None, None
    with np.errstate(invalid="ignore"):
        w = Rows((pa[:, 0] - ca[0]) * sa, (pa[:, 1] - ca[1]) * sa, (pb[:, 0] - cb[0]) * sb, (pb[:, 1] - cb[1]) * sb, sa, sb)
    Mn = None
    M = np.asarray(M, dtype=np.float64)
    if np.isfinite(M).all():
        L, Rm, _, _ = transforms(model, ca, sa, cb, sb)
        Mn = mat3(mat3(L, M), Rm)
        f = fro(Mn)
        Mn = Mn / f if f > 0 and math.isfinite(f) else None
    return w, Mn, (ca, sa, cb, sb)


def pixel_cost(model, M, pa, pb, thr):
    """(truncated cost, active rows [n]) of the pixel model M: the direct evaluation the tests compare `cost` with"""
    w, Mn, _ = prepare(model, M, pa, pb)
    fit = FITS[model]
    return truncated(fit.residuals(fit.init(Mn), w), thr)


def refine(model, M, pa, pb, thr, max_steps=25, valid=True):
    """One pair.  Returns a dict: M [3, 3], mask [n], info = (accepted steps, cost evaluations, active rows at the end, pair
    fitted), cost0, cost."""
    fit = FITS[model]
    M = np.array(M, dtype=np.float64).reshape(3, 3)
    n = len(np.asarray(pa).reshape(-1, 2))
    out = dict(M=M, mask=np.zeros(n, dtype=bool), info=(0, 0, 0, 0), cost0=math.nan, cost=math.nan)
    if not (bool(valid) and n >= fit.MIN_ROWS and thr > 0):
        return out
    w, Mn, nrm = prepare(model, M, pa, pb)
    st = fit.init(Mn) if Mn is not None else None
    if st is None:
        return out
    st, steps, evals, a, cost0, cur = lm_ref.fit(fit, st, w, thr, max_steps)
    out.update(M=denormalise(model, fit.matrix(st), *nrm) if steps else M, mask=a, info=(steps, evals, int(a.sum()), 1),
               cost0=cost0, cost=cur)
    return out


def refine_homography(H, pa, pb, thr, max_steps=25):
    """roma_amd.refine_homography for one pair: (H, mask, info, (cost0, cost))"""
    o = refine(HOMOGRAPHY, H, pa, pb, thr, max_steps)
    return o["M"], o["mask"], o["info"], (o["cost0"], o["cost"])


def refine_fundamental(F, pa, pb, thr, max_steps=25):
    """roma_amd.refine_fundamental for one pair: (F, mask, info, (cost0, cost))"""
    o = refine(FUNDAMENTAL, F, pa, pb, thr, max_steps)
    return o["M"], o["mask"], o["info"], (o["cost0"], o["cost"])
