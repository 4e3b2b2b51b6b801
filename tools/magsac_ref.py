"""numpy float64 restatement of the device MAGSAC++ scoring of homography and fundamental-matrix RANSAC (csrc/ransac.h magsac_*,
csrc/geometry.hip, `roma_amd.geometry.magsac`): the oracle of tests/test_gpu_magsac.py.

MAGSAC++ (Barath et al., CVPR 2020) with nu = 4 degrees of freedom.  threshold tau is the largest residual that counts as an
inlier; k^2 = 13.276704135987625 is the 0.99 quantile of chi^2 with 4 DoF, sigma_max = tau / k, and a residual r (pixels) has
V = r^2 / (2 sigma_max^2), V_k = k^2 / 2.  The dimensionless loss and the IRLS weight are

    rho(V) = gamma(5/2, V) + V (Gamma(3/2, V) - Gamma(3/2, V_k))    V < V_k
    rho(V) = gamma(5/2, V_k)                                         V >= V_k and non-finite rows
    w(V)   = Gamma(3/2, V) - Gamma(3/2, V_k)                         V < V_k, else 0

(the MAGSAC++ loss up to the positive factor sigma_max 2^{3/2} / 4; rho(0) = 0, rho is continuous at V_k and d rho / dV = w), in
closed form through erfc / erf.  Residuals: forward reprojection error in image B (H), Sampson distance (F), both evaluated from
the Hartley-normalised points without de-normalising.

Per pair: the sampling rounds of tools/geometry_ref.py (same samples, same minimal solvers), each model scored by its sum of rho
over the pair's rows; the smallest score of a round (ties: lowest (h, slot)) replaces the running best if strictly smaller;
OpenCV's adaptive iteration count on the inlier ratio #{r < tau} / n of the new best.  After sampling up to lo_iters IRLS steps:
the weights w under the current model, the weighted normal equations sum w_i a_i a_i^T (the rows of geometry_ref.refit),
smallest eigenvector, rank 2 for F; the candidate is kept only if its score is strictly lower - the gain sum(rho_cur - rho_cand)
measured paired, the candidate's residual terms as the current model's plus those of (cand - cur) (lo_gain) - else LO stops;
LO also stops with fewer than REFIT_MIN rows of positive weight.  The final score is the winning minimal model's less the gains.
Mask: r < tau under the final model.

Differences by design: the device evaluates residuals and rho in f32 and sums in f32 (`f32=True` here evaluates r^2 in float32
with the device's operation order, the rest stays f64), and the refit's eigenvector / rank-2 step use LAPACK here and one-sided
Jacobi on the device.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import geometry_ref as gr

HOMOGRAPHY, FUNDAMENTAL = gr.HOMOGRAPHY, gr.FUNDAMENTAL
K2 = 13.276704135987625            # 0.99 quantile of chi^2, 4 DoF
VK = K2 / 2                        # 6.638352067993813
GAMMA32_K = 0.003611260617758621   # Gamma(3/2, V_k)
RHO_MAX = 1.3015316073311316       # gamma(5/2, V_k)
LO_ITERS = 10


def _erfc(x):
    return torch.special.erfc(torch.from_numpy(np.asarray(x, dtype=np.float64))).numpy()


def _erf(x):
    return torch.special.erf(torch.from_numpy(np.asarray(x, dtype=np.float64))).numpy()


def upper_gamma_32(x):
    """Gamma(3/2, x) = 1/2 Gamma(1/2, x) + sqrt(x) e^-x with Gamma(1/2, x) = sqrt(pi) erfc(sqrt(x))"""
    s = np.sqrt(x)
    return 0.5 * math.sqrt(math.pi) * _erfc(s) + s * np.exp(-x)


def lower_gamma_52(x):
    """gamma(5/2, x) = 3/2 gamma(3/2, x) - x^{3/2} e^-x with gamma(3/2, x) = 1/2 sqrt(pi) erf(sqrt(x)) - sqrt(x) e^-x"""
    s = np.sqrt(x)
    g32 = 0.5 * math.sqrt(math.pi) * _erf(s) - s * np.exp(-x)
    return 1.5 * g32 - x * s * np.exp(-x)


def loss(V):
    """(rho(V), w(V)) elementwise; V >= V_k and non-finite V give (RHO_MAX, 0)"""
    V = np.asarray(V, dtype=np.float64)
    inside = V < VK  # False for NaN
    Vi = np.where(inside, V, 0.0)
    w = upper_gamma_32(Vi) - GAMMA32_K
    rho = lower_gamma_52(Vi) + Vi * w
    return np.where(inside, rho, RHO_MAX), np.where(inside, w, 0.0)


def _ops(f32):
    """(round, fma): identity and a * b + c in f64, or rounding to float32 after every operation (the product of two float32
    values is exact in f64, so round(a * b + c) is the device's fmaf up to a double rounding)"""
    if not f32:
        return (lambda x: x), (lambda a, b, c: a * b + c)

    def r(x):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)
    return r, (lambda a, b, c: r(a * b + c))


def res_terms(model, M, xa, xb, f32=False):
    """the residual terms linear in the model, [NT, K, n], of models M [K, 3, 3] (normalised) on normalised points xa, xb [n, 2]:
    (e_x, e_y, p_z) for H, (d, l_x, l_y, k_x, k_y) for F.  f32: the device's float32 evaluation, in its operation order"""
    r, fma = _ops(f32)
    m = r(M.reshape(-1, 9))[:, :, None]
    x, y, u, v = (r(c)[None] for c in (xa[:, 0], xa[:, 1], xb[:, 0], xb[:, 1]))
    with np.errstate(all="ignore"):
        if model == HOMOGRAPHY:
            px = fma(m[:, 0], x, fma(m[:, 1], y, m[:, 2]))
            py = fma(m[:, 3], x, fma(m[:, 4], y, m[:, 5]))
            pz = fma(m[:, 6], x, fma(m[:, 7], y, m[:, 8]))
            return np.stack([fma(-u, pz, px), fma(-v, pz, py), pz])
        lx = fma(m[:, 0], x, fma(m[:, 1], y, m[:, 2]))
        ly = fma(m[:, 3], x, fma(m[:, 4], y, m[:, 5]))
        lz = fma(m[:, 6], x, fma(m[:, 7], y, m[:, 8]))
        return np.stack([fma(u, lx, fma(v, ly, lz)), lx, ly, fma(m[:, 0], u, fma(m[:, 3], v, m[:, 6])),
                         fma(m[:, 1], u, fma(m[:, 4], v, m[:, 7]))])


def r2_from(model, t, sa, sb, f32=False):
    """squared pixel residuals from the terms of res_terms: |e|^2 / (p_z^2 s_b^2) (H), d^2 / (s_b^2 |l|^2 + s_a^2 |k|^2) (F)"""
    r, fma = _ops(f32)
    sa2, sb2 = r(sa * sa), r(sb * sb)
    with np.errstate(all="ignore"):
        if model == HOMOGRAPHY:
            ex, ey, pz = t
            return r(fma(ex, ex, r(ey * ey)) / r(r(pz * pz) * sb2))
        d, lx, ly, kx, ky = t
        return r(r(d * d) / fma(sb2, fma(lx, lx, r(ly * ly)), r(sa2 * fma(kx, kx, r(ky * ky)))))


def residual2(model, M, xa, xb, sa, sb, f32=False):
    """squared pixel residuals [K, n] of models M [K, 3, 3] (normalised) on normalised points xa, xb [n, 2]: forward reprojection
    error in image B (H), Sampson distance (F).  f32: the device's float32 evaluation, in its operation order"""
    return r2_from(model, res_terms(model, M, xa, xb, f32), sa, sb, f32)


def lo_gain(terms, r2_of, cur, cand, vs, f32=False):
    """sum(rho_cur - rho_cand) over the rows, measured paired as the device does: the candidate's residual terms are the current
    model's plus those of the difference (cand - cur), so the error both share cancels.  terms(M [1, 3, 3]) -> the residual
    terms, r2_of(terms) -> the squared residuals"""
    r, _ = _ops(f32)
    tu = terms(cur[None])
    tc = r(tu + terms((cand - cur)[None]))
    with np.errstate(invalid="ignore"):
        return float((loss(r2_of(tu) * vs)[0] - loss(r2_of(tc) * vs)[0]).sum())


def weighted_refit(model, xa, xb, w):
    """the weighted normal equations sum w_i a_i a_i^T over the rows of geometry_ref.refit that have positive weight: smallest
    eigenvector, rank 2 for F, unit norm"""
    sel = w > 0
    x, y, u, v = xa[sel, 0], xa[sel, 1], xb[sel, 0], xb[sel, 1]
    ws = w[sel]
    one, zero = np.ones_like(x), np.zeros_like(x)
    if model == HOMOGRAPHY:
        A = np.concatenate([np.stack([x, y, one, zero, zero, zero, -u * x, -u * y, -u], 1),
                            np.stack([zero, zero, zero, x, y, one, -v * x, -v * y, -v], 1)])
        ws = np.concatenate([ws, ws])
    else:
        A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, one], 1)
    _, vec = np.linalg.eigh((A * ws[:, None]).T @ A)
    h = vec[:, 0].reshape(3, 3)
    if model == FUNDAMENTAL:
        U, S, Vt = np.linalg.svd(h)
        h = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    return h / np.linalg.norm(h)


def minimal_model(model, pa, pb, seed, h, root):
    """the normalised minimal model of hypothesis h, slot root (None if it does not exist)"""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    ca, sa, cb, sb, fin, cnt = gr.normalize(pa, pb)
    with np.errstate(invalid="ignore"):
        xa, xb = (pa - ca) * sa, (pb - cb) * sb
    idx, drawn = gr.draw_samples(seed, [h], len(pa), gr.SAMPLE[model])
    if not (drawn[0] and fin[idx[0]].all()):
        return None
    if model == HOMOGRAPHY:
        H, ok = gr.solve_h(xa[idx], xb[idx])
        return H[0] if ok[0] and root == 0 else None
    F, nm = gr.solve_f(xa[idx], xb[idx])
    return F[0, root] if root < nm[0] else None


def scores(model, pa, pb, thr, Ms, f32=False):
    """per model of Ms [K, 3, 3] (normalised) on the pair: (sum of rho [K], rho [K, n], w [K, n], V [K, n])"""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    ca, sa, cb, sb, fin, cnt = gr.normalize(pa, pb)
    with np.errstate(invalid="ignore"):
        xa, xb = (pa - ca) * sa, (pb - cb) * sb
        V = residual2(model, Ms, xa, xb, sa, sb, f32) * (K2 / (2 * float(thr) ** 2))
    rho, w = loss(V)
    return rho.sum(axis=1), rho, w, V


def run(out, name, n, s, slots, fin, seed, conf, max_iters, lo_iters, t2, solve, terms, r2_of, refit, finish, f32=False):
    """what the MAGSAC++ oracles (`magsac` here, essential_magsac_ref.magsac) share once the pair is normalised: the sampling
    rounds (geometry_ref.round_loop on the smallest sum of rho), the LO loop with its paired gain, the result dict.  t2: squared
    threshold in the units of the residual; solve: round_loop's; terms(Ms [K, 3, 3]) -> residual terms and r2_of(terms) ->
    squared residuals [K, n]; refit(w [n], score) -> an IRLS candidate or None (score(Ms) -> sums of rho); finish(cur) -> the
    model returned as out[name].  Fills and returns out."""
    vs = K2 / (2 * t2)

    def residual2(Ms):
        return r2_of(terms(Ms))

    def score(Ms):
        r2 = residual2(Ms)
        with np.errstate(invalid="ignore"):
            return loss(r2 * vs)[0].sum(axis=1), (r2 < t2).sum(axis=1)

    score_min, best, cur, best_h, best_root, rounds = gr.round_loop(n, s, slots, fin, seed, conf, max_iters, solve, score, smaller=True)
    out.update(rounds=rounds, best_h=best_h, best_root=best_root, best_min=best)
    if cur is None:
        return out
    gains, lo_steps = 0.0, 0
    for _ in range(lo_iters):
        with np.errstate(invalid="ignore"):
            w = np.maximum(loss(residual2(cur[None])[0] * vs)[1], 0.0)
        cand = refit(w, lambda Ms: score(Ms)[0])
        if cand is None:
            break
        gain = lo_gain(terms, r2_of, cur, cand, vs, f32)
        if not gain > 0:
            break
        cur, gains, best, lo_steps = cand, gains + gain, int(score(cand[None])[1][0]), lo_steps + 1
    out.update(best=best, score_min=score_min, score=score_min - gains, lo_steps=lo_steps)
    if best <= 0:
        return out
    with np.errstate(invalid="ignore"):
        mask = residual2(cur[None])[0] < t2
    out.update({name: finish(cur)}, mask=mask, ok=True)
    return out


def magsac(model, pa, pb, thr, conf, max_iters, seed, lo_iters=LO_ITERS, f32=False):
    """One pair.  pa, pb [n, 2] pixels (rows of the pair only).  Returns a dict with geometry_ref.ransac's fields (M [3, 3] or
    zeros, mask [n], ok, rounds, best_h, best_root, best_min = inliers of the winning minimal model, best = final inliers) plus
    score_min (sum of rho of the winning minimal model), score (final sum of rho: score_min less the LO gains; both 0 where no model) and lo_steps."""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    n, s = len(pa), gr.SAMPLE[model]
    out = dict(M=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), ok=False, rounds=0, best_h=-1, best_root=-1, best_min=-1,
               best=-1, score_min=0.0, score=0.0, lo_steps=0)
    if n < s:
        return out
    ca, sa, cb, sb, fin, cnt = gr.normalize(pa, pb)
    if not (cnt >= s and math.isfinite(sa) and math.isfinite(sb)):
        return out
    with np.errstate(invalid="ignore"):
        xa, xb = (pa - ca) * sa, (pb - cb) * sb

    def solve(idx):
        if model == HOMOGRAPHY:
            H, ok = gr.solve_h(xa[idx], xb[idx])
            return H[:, None], ok.astype(np.int64)
        return gr.solve_f(xa[idx], xb[idx])

    def refit(w, score):
        if int((w > 0).sum()) < gr.REFIT_MIN[model]:
            return None
        cand = weighted_refit(model, xa, xb, w)
        return cand if np.isfinite(cand).all() else None

    return run(out, "M", n, s, gr.SLOTS[model], fin, seed, conf, max_iters, lo_iters, float(thr) ** 2, solve,
               lambda Ms: res_terms(model, Ms, xa, xb, f32), lambda t: r2_from(model, t, sa, sb, f32), refit,
               lambda cur: gr.denormalise(model, cur, ca, sa, cb, sb), f32)
