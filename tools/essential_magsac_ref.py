"""numpy float64 restatement of the device MAGSAC++ scoring and local optimisation of essential-matrix RANSAC
(csrc/ransac.h magsac_*, csrc/essential.hip Essential::residual2 / wrefit, `roma_amd.geometry.essential_magsac`): the oracle of
tests/test_gpu_essential_magsac.py.  It builds on tools/essential_ref.py (normalisation, sampling, `five_point`) and on
tools/magsac_ref.py (`loss`, the weights, the f32 operation model).

Per pair: the camera normalisation and the sampling rounds of essential_ref.ransac (same samples, same five-point models, up to
ten slots per hypothesis), each model scored by its sum of rho(V) over the pair's rows, V = r^2 k^2 / (2 tau^2) with r^2 the
squared Sampson distance in normalised camera coordinates, d^2 / ((l_x^2 + l_y^2) + (k_x^2 + k_y^2)) - the expression of
essential_ref.inliers, so r^2 < tau^2 is find_essential's inlier rule - and tau = threshold / ((fx + fy) / 2).  The smallest
score of a round (ties: lowest (h, slot)) replaces the running best if strictly smaller; OpenCV's adaptive iteration count on
#{r < tau} / n of the new best.  After sampling up to lo_iters IRLS steps (weighted_refit): the MAGSAC++ weights w under the
current model; over the rows of positive weight (at least 8) Hartley normalisation of both images and the weighted eight-point
normal equations sum w_i a_i a_i^T; the eigenvectors of their four smallest eigenvalues, de-normalised, as the basis X, Y, Z, W
of the five-point solver's cubic constraints (Nister's form for more than five points); of its solutions the one of the
smallest score, projected onto the essential manifold (singular values ((s1 + s2) / 2, (s1 + s2) / 2, 0)), unit Frobenius norm,
largest-magnitude entry positive.  The candidate is kept only if its score is strictly lower - the gain measured paired as in
magsac_ref.lo_gain - else LO stops.  Mask: r < tau under the final E.

Differences by design: those of magsac_ref (`f32=True` evaluates r^2 in float32 in the device's operation order; LAPACK's
eigenvectors and SVD here, one-sided Jacobi on the device).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_ref as er  # noqa: E402
import geometry_ref as gr  # noqa: E402
import magsac_ref as mr  # noqa: E402

LO_ITERS = 10
REFIT_MIN = 8  # rows of positive weight the eight-point step needs


def r2_from(t, f32=False):
    """squared Sampson distance from the terms (d, l_x, l_y, k_x, k_y) of magsac_ref.res_terms(FUNDAMENTAL, ...)"""
    r, fma = mr._ops(f32)
    d, lx, ly, kx, ky = t
    with np.errstate(all="ignore"):
        return r(r(d * d) / r(fma(lx, lx, r(ly * ly)) + fma(kx, kx, r(ky * ky))))


def residual2(E, xa, xb, f32=False):
    """squared Sampson distances [K, n] of models E [K, 3, 3] on normalised points xa, xb [n, 2]; f32: the device's float32
    evaluation, in its operation order"""
    return r2_from(mr.res_terms(mr.FUNDAMENTAL, E, xa, xb, f32), f32)


def project(F):
    """the closest essential matrix in the Frobenius norm: singular values ((s1 + s2) / 2, (s1 + s2) / 2, 0); then unit norm and
    the sign rule of five_point (largest-magnitude entry positive, the first one on ties)"""
    U, S, Vt = np.linalg.svd(F)
    s = 0.5 * (S[0] + S[1])
    E = U @ np.diag([s, s, 0.0]) @ Vt
    with np.errstate(all="ignore"):
        E = E / np.linalg.norm(E)
    return E * (-1.0 if E.flat[int(np.argmax(np.abs(E)))] < 0 else 1.0)


def refit_basis(xa, xb, w):
    """the least-squares null space of one IRLS step, [9, 4] = X, Y, Z, W (W belongs to the smallest eigenvalue): over the rows
    of positive weight Hartley normalisation of both images, the weighted eight-point normal equations sum w_i a_i a_i^T, the
    eigenvectors of their four smallest eigenvalues, de-normalised (Tb^T F_n Ta) and orthonormalised by modified Gram-Schmidt in
    the order X, Y, Z, W.  None with fewer than REFIT_MIN such rows or a normalisation that is not finite."""
    sel = w > 0
    if int(sel.sum()) < REFIT_MIN:
        return None
    a, b, ws = xa[sel], xb[sel], w[sel]
    cnt = len(a)
    ca, cb = a.sum(axis=0) / cnt, b.sum(axis=0) / cnt
    ma, mb = np.sqrt(((a - ca) ** 2).sum(axis=1)).sum() / cnt, np.sqrt(((b - cb) ** 2).sum(axis=1)).sum() / cnt
    if not (ma > 0 and mb > 0):
        return None
    sa, sb = math.sqrt(2) / ma, math.sqrt(2) / mb
    if not (math.isfinite(sa) and math.isfinite(sb)):
        return None
    x, y, u, v = (a[:, 0] - ca[0]) * sa, (a[:, 1] - ca[1]) * sa, (b[:, 0] - cb[0]) * sb, (b[:, 1] - cb[1]) * sb
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 1)
    _, vec = np.linalg.eigh((A * ws[:, None]).T @ A)  # ascending eigenvalues
    Ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1]])
    Tbt = np.array([[sb, 0, 0], [0, sb, 0], [-sb * cb[0], -sb * cb[1], 1]])
    basis = np.zeros((9, 4))
    with np.errstate(all="ignore"):
        for f in range(4):
            q = (Tbt @ vec[:, 3 - f].reshape(3, 3) @ Ta).reshape(9)
            for g in range(f):
                q = q - (q @ basis[:, g]) * basis[:, g]
            basis[:, f] = q / math.sqrt(q @ q)
    return basis


def weighted_refit(xa, xb, w, score):
    """one IRLS step on normalised camera coordinates xa, xb [n, 2] with weights w [n]: the five-point solver's cubic constraints
    on refit_basis - Nister's form for more than five points, the E of the least-squares null space that are essential
    matrices - and of its solutions the one of the smallest score(Es [K, 3, 3]) -> [K] (the first on ties), projected onto the
    essential manifold.  None without a basis or a solution.

    The smallest eigenvector alone, projected, is the eight-point algorithm.  The relief scenes are close to a plane, where
    the eight-point system has a null space of more than one dimension and its smallest eigenvector follows the noise: on the
    24 noisy cases of tests/test_cpu_pose_refine.py that candidate lowered the score of the winning five-point model in 4 cases
    and the pose error in 2 of them."""
    basis = refit_basis(xa, xb, w)
    if basis is None:
        return None
    Es, n = er.solve_basis(basis[None], np.ones(1, dtype=bool))
    if n[0] == 0:
        return None
    E = project(Es[0, int(np.argmin(score(Es[0, :n[0]])))])
    return E if np.isfinite(E).all() else None


def _pair(pa, pb, thr, K):
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    thr_n = float(thr) if K is None else float(thr) / ((K[0, 0] + K[1, 1]) * 0.5)
    fin = np.isfinite(pa).all(axis=1) & np.isfinite(pb).all(axis=1)
    with np.errstate(invalid="ignore"):
        xa, xb = er._normalise(pa, K), er._normalise(pb, K)
    return xa, xb, fin, thr_n * thr_n


def _round_models(xa, xb, fin, seed, rd):
    """the five-point models of sampling round rd: ([ROUND, MAX_ROOTS, 3, 3], number of models [ROUND])"""
    idx, drawn = gr.draw_samples(seed, np.arange(rd * gr.ROUND, (rd + 1) * gr.ROUND), len(xa), 5)
    idx = np.where(drawn[:, None], idx, 0)
    ok = drawn & fin[idx].all(axis=1)
    models = np.zeros((gr.ROUND, er.MAX_ROOTS, 3, 3))
    nm = np.zeros(gr.ROUND, dtype=np.int64)
    sel = np.nonzero(ok)[0]
    if len(sel):
        models[sel], nm[sel] = er.five_point(xa[idx[sel]], xb[idx[sel]])
    return models, nm


def minimal_model(pa, pb, seed, h, root, K=None):
    """the five-point model of hypothesis h, slot root (None if it does not exist), solved with its round as `magsac` solves it
    (numpy's batched kernels round by batch shape)"""
    xa, xb, fin, _ = _pair(pa, pb, 1.0, K)
    models, nm = _round_models(xa, xb, fin, seed, h // gr.ROUND)
    return models[h % gr.ROUND, root].copy() if 0 <= root < nm[h % gr.ROUND] else None


def scores(pa, pb, thr, Es, K=None, f32=False):
    """per model of Es [M, 3, 3] on the pair: (sum of rho [M], rho [M, n], w [M, n], V [M, n])"""
    xa, xb, fin, t2 = _pair(pa, pb, thr, K)
    with np.errstate(invalid="ignore"):
        V = residual2(np.asarray(Es, dtype=np.float64), xa, xb, f32) * (mr.K2 / (2 * t2))
    rho, w = mr.loss(V)
    return rho.sum(axis=1), rho, w, V


def magsac(pa, pb, thr, prob, max_iters, seed, K=None, lo_iters=LO_ITERS, f32=False):
    """One pair.  pa, pb [n, 2] (rows of the pair only; what the device reads, i.e. f32-rounded); K a camera matrix or None
    (normalised points).  Returns a dict: E [3, 3] (or zeros), mask [n], ok, rounds, best_h, best_root, best_min = inliers of the
    winning minimal model, best = final inliers, score_min (sum of rho of the winning minimal model), score (final sum: score_min
    less the LO gains; both 0 where no model), lo_steps."""
    n = len(pa)
    out = dict(E=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), ok=False, rounds=0, best_h=-1, best_root=-1, best_min=-1, best=-1,
               score_min=0.0, score=0.0, lo_steps=0)
    xa, xb, fin, t2 = _pair(pa, pb, thr, K)
    if n < 5 or fin.sum() < 5 or not (t2 > 0 and math.isfinite(t2)):
        return out
    return mr.run(out, "E", n, 5, er.MAX_ROOTS, fin, seed, prob, max_iters, lo_iters, t2,
                  lambda idx: er.five_point(xa[idx], xb[idx]), lambda Ms: mr.res_terms(mr.FUNDAMENTAL, Ms, xa, xb, f32),
                  lambda t: r2_from(t, f32), lambda w, score: weighted_refit(xa, xb, w, score), lambda cur: cur, f32)


def estimate_pose(kpts0, kpts1, K0, K1, norm_thresh, conf=0.99999, max_iters=1000, seed=0, lo_iters=LO_ITERS, f32=False):
    """essential_ref.estimate_pose with `magsac` in place of `ransac`: (R, t [3, 1], mask) or None"""
    if len(kpts0) < 5:
        return None
    K0inv, K1inv = np.linalg.inv(K0[:2, :2]), np.linalg.inv(K1[:2, :2])
    x0 = (K0inv @ (np.asarray(kpts0, dtype=np.float64) - K0[None, :2, 2]).T).T.astype(np.float32).astype(np.float64)
    x1 = (K1inv @ (np.asarray(kpts1, dtype=np.float64) - K1[None, :2, 2]).T).T.astype(np.float32).astype(np.float64)
    r = magsac(x0, x1, norm_thresh, conf, max_iters, seed, None, lo_iters, f32)
    if not r["ok"]:
        return None
    n, R, t, good = er.recover_pose(r["E"], x0, x1, r["mask"])
    if n == 0:
        return None
    return R, t, good
