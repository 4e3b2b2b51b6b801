"""numpy float64 restatement of the device RANSAC (roma_amd/csrc/geometry.hip, `roma_amd.geometry`): the oracle of
tests/test_gpu_geometry.py, in the way tools/pose_geometry.py is the oracle of the pose harness.

Same algorithm step by step: Hartley normalisation per image, hypotheses in rounds of ROUND per pair drawn by the same
counter-based generator (the splitmix64 finaliser of csrc/sampling.h on (seed, h, draw)), the same minimal solvers (4-point DLT
as an 8 x 8 Gauss-Jordan solve with OpenCV's checkSubset; 7-point null space + closed-form cubic), the same inlier tests, the
same selection (largest count, ties to the lowest (h, root)), OpenCV's adaptive iteration count with the ceiling of the ratio,
and the same refinement (least-squares refit on the inliers, kept if its count is not lower).  Differences by design: the
device scores in f32 (here f64, so masks can differ at points whose error lies at the threshold), and the refit's smallest
eigenvector / rank-2 step use LAPACK here and one-sided Jacobi on the device.
"""
from __future__ import annotations

import math

import numpy as np

HOMOGRAPHY, FUNDAMENTAL = 0, 1
ROUND = 256
MAX_ROOTS = 3
MAX_TRY = 64
REFINE_ITERS = 3
COLLINEAR_EPS = 1e-4
PIVOT_EPS = 1e-6
CUBIC_EPS = 1e-12
SAMPLE = {HOMOGRAPHY: 4, FUNDAMENTAL: 7}
REFIT_MIN = {HOMOGRAPHY: 4, FUNDAMENTAL: 8}
SLOTS = {HOMOGRAPHY: 1, FUNDAMENTAL: MAX_ROOTS}  # models per hypothesis
_G1, _G2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD1B54A32D192ED03)


def mix64(z):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_samples(seed, hs, n, s):
    """indices [len(hs), s] of hypotheses hs and whether each sample was drawn: draw j takes mix64(key_h + G2 (c + 1)) mod n with
    c = j, j + s, j + 2 s, ... (at most MAX_TRY tries) until it differs from the draws before it; key_h = mix64(seed + G1 (h + 1))"""
    hs = np.asarray(hs, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = mix64(np.uint64(seed) + _G1 * (hs + np.uint64(1)))
    idx = np.full((len(hs), s), -1, dtype=np.int64)
    ok = np.ones(len(hs), dtype=bool)
    for j in range(s):
        got = np.zeros(len(hs), dtype=bool)
        for t in range(MAX_TRY):
            c = np.uint64(j + t * s)
            with np.errstate(over="ignore"):
                v = (mix64(key + _G2 * (c + np.uint64(1))) % np.uint64(n)).astype(np.int64)
            take = ~got & ~(idx[:, :j] == v[:, None]).any(axis=1)
            idx[take, j] = v[take]
            got |= take
            if got.all():
                break
        ok &= got
    return idx, ok


def normalize(pa, pb):
    """Hartley normalisation over the finite rows: (ca, sa, cb, sb, finite rows, valid) with x_n = (x - c) * s"""
    fin = np.isfinite(pa).all(axis=1) & np.isfinite(pb).all(axis=1)
    cnt = int(fin.sum())
    if cnt == 0:
        return None, np.nan, None, np.nan, fin, cnt
    ca, cb = pa[fin].sum(axis=0) / cnt, pb[fin].sum(axis=0) / cnt
    ma = np.sqrt(((pa[fin] - ca) ** 2).sum(axis=1)).sum() / cnt
    mb = np.sqrt(((pb[fin] - cb) ** 2).sum(axis=1)).sum() / cnt
    with np.errstate(divide="ignore"):
        sa, sb = math.sqrt(2) / ma if ma > 0 else np.inf, math.sqrt(2) / mb if mb > 0 else np.inf
    return ca, sa, cb, sb, fin, cnt


def gauss_jordan(a):
    """batched Gauss-Jordan with partial pivoting (first maximum) of the pivot columns 0 .. rows-1: (reduced a, ok)"""
    a = np.array(a, dtype=np.float64)
    m, rows, _ = a.shape
    ar = np.arange(m)
    ok = np.ones(m, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(rows):
            col = np.abs(a[:, k:, k])
            p = k + np.argmax(col, axis=1)
            ok &= col[ar, p - k] > PIVOT_EPS
            rk, rp = a[ar, k].copy(), a[ar, p].copy()
            a[ar, k], a[ar, p] = rp, rk
            inv = 1.0 / a[:, k, k]
            a[:, k, :] = a[:, k, :] * inv[:, None]
            for r in range(rows):
                if r != k:
                    f = a[:, r, k].copy()
                    a[:, r, :] = a[:, r, :] - f[:, None] * a[:, k, :]
    return a, ok


def h_subset_ok(xa, xb):
    """OpenCV's checkSubset on samples [M, 4, 2]: no (nearly) collinear triple in either image, and the four triples all keep
    or all flip their orientation"""
    neg = np.zeros(len(xa), dtype=np.int64)
    ok = np.ones(len(xa), dtype=bool)
    for i, j, k in ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)):
        cr = []
        for x in (xa, xb):
            d1, d2 = x[:, j] - x[:, i], x[:, k] - x[:, i]
            c = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
            ok &= np.abs(c) > COLLINEAR_EPS * np.sqrt((d1[:, 0] ** 2 + d1[:, 1] ** 2) * (d2[:, 0] ** 2 + d2[:, 1] ** 2))
            cr.append(c)
        neg += cr[0] * cr[1] < 0
    return ok & ((neg == 0) | (neg == 4))


def solve_h(xa, xb):
    """4-point DLT on samples [M, 4, 2] (normalised): (H [M, 3, 3] with H[2, 2] = 1, ok [M])"""
    m = len(xa)
    x, y, u, v = xa[..., 0], xa[..., 1], xb[..., 0], xb[..., 1]
    a = np.zeros((m, 8, 9))
    a[:, 0::2, 0], a[:, 0::2, 1], a[:, 0::2, 2] = x, y, 1
    a[:, 0::2, 6], a[:, 0::2, 7], a[:, 0::2, 8] = -u * x, -u * y, u
    a[:, 1::2, 3], a[:, 1::2, 4], a[:, 1::2, 5] = x, y, 1
    a[:, 1::2, 6], a[:, 1::2, 7], a[:, 1::2, 8] = -v * x, -v * y, v
    r, ok = gauss_jordan(a)
    H = np.concatenate([r[:, :, 8], np.ones((m, 1))], axis=1).reshape(m, 3, 3)
    return H, ok & h_subset_ok(xa, xb) & np.isfinite(H).all(axis=(1, 2))


def det3(f):
    return f[..., 0] * (f[..., 4] * f[..., 8] - f[..., 5] * f[..., 7]) - f[..., 1] * (f[..., 3] * f[..., 8] - f[..., 5] * f[..., 6]) \
        + f[..., 2] * (f[..., 3] * f[..., 7] - f[..., 4] * f[..., 6])


def solve_cubic(c3, c2, c1, c0):
    """real roots of c3 x^3 + c2 x^2 + c1 x + c0, ascending (closed form, then two Newton steps)"""
    cmax = max(abs(c3), abs(c2), abs(c1), abs(c0))
    if not (cmax > 0) or not math.isfinite(cmax):
        return []
    if abs(c3) <= CUBIC_EPS * cmax:
        if abs(c2) <= CUBIC_EPS * cmax:
            if abs(c1) <= CUBIC_EPS * cmax:
                return []
            x = [-c0 / c1]
        else:
            d = c1 * c1 - 4 * c2 * c0
            if d < 0:
                return []
            q = -0.5 * (c1 + math.copysign(math.sqrt(d), c1))
            r0 = q / c2
            r1 = c0 / q if q != 0 else r0
            x = [min(r0, r1), max(r0, r1)]
    else:
        a, b, c = c2 / c3, c1 / c3, c0 / c3
        Q, R = (a * a - 3 * b) / 9, (2 * a * a * a - 9 * a * b + 27 * c) / 54
        Q3 = Q * Q * Q
        if R * R < Q3:
            th, sq, a3 = math.acos(R / math.sqrt(Q3)), -2 * math.sqrt(Q), a / 3
            x = [sq * math.cos(th / 3) - a3, sq * math.cos((th + 2 * math.pi) / 3) - a3, sq * math.cos((th - 2 * math.pi) / 3) - a3]
        else:
            A = -math.copysign(np.cbrt(abs(R) + math.sqrt(R * R - Q3)), R)
            Bq = Q / A if A != 0 else 0.0
            x = [(A + Bq) - a / 3]
    out = []
    for r in x:
        for _ in range(2):
            p, dp = ((c3 * r + c2) * r + c1) * r + c0, (3 * c3 * r + 2 * c2) * r + c1
            if dp != 0:
                r1 = r - p / dp
                if math.isfinite(r1):
                    r = r1
        out.append(float(r))
    return sorted(out)


def solve_f(xa, xb):
    """7-point solver on samples [M, 7, 2] (normalised): (F [M, 3, 3, 3] unit Frobenius norm, number of models [M]); model r of
    sample i is F[i, r] for r < n[i], in ascending order of alpha in det(alpha F1 + (1 - alpha) F2) = 0"""
    m = len(xa)
    x, y, u, v = xa[..., 0], xa[..., 1], xb[..., 0], xb[..., 1]
    a = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], axis=-1)
    r, ok = gauss_jordan(a)
    F = np.zeros((m, MAX_ROOTS, 9))
    n = np.zeros(m, dtype=np.int64)
    for i in np.nonzero(ok)[0]:
        f1 = np.r_[-r[i, :, 7], 1.0, 0.0]
        f2 = np.r_[-r[i, :, 8], 0.0, 1.0]
        d = f1 - f2
        g = f2 - d
        c0, c3, p1, pm1 = det3(f2), det3(d), det3(f1), det3(g)
        c2, c1 = (p1 + pm1) * 0.5 - c0, (p1 - pm1) * 0.5 - c3
        for al in solve_cubic(c3, c2, c1, c0):
            f = al * f1 + (1 - al) * f2
            with np.errstate(all="ignore"):
                f = f * (1.0 / math.sqrt(float((f * f).sum())))
            if np.isfinite(f).all():
                F[i, n[i]] = f
                n[i] += 1
    return F.reshape(m, MAX_ROOTS, 3, 3), n


def inliers(model, M, xa, xb, t2a, t2b):
    """inlier masks [K, n] of models M [K, 3, 3] (normalised) on points xa, xb [n, 2] (normalised; NaN never passes)"""
    m = M.reshape(-1, 9)[:, :, None]
    x, y, u, v = xa[None, :, 0], xa[None, :, 1], xb[None, :, 0], xb[None, :, 1]
    with np.errstate(invalid="ignore"):
        if model == HOMOGRAPHY:
            px, py, pz = m[:, 0] * x + m[:, 1] * y + m[:, 2], m[:, 3] * x + m[:, 4] * y + m[:, 5], m[:, 6] * x + m[:, 7] * y + m[:, 8]
            ex, ey = px - u * pz, py - v * pz
            return ex * ex + ey * ey < t2b * (pz * pz)
        lx, ly, lz = m[:, 0] * x + m[:, 1] * y + m[:, 2], m[:, 3] * x + m[:, 4] * y + m[:, 5], m[:, 6] * x + m[:, 7] * y + m[:, 8]
        d = u * lx + v * ly + lz
        kx, ky = m[:, 0] * u + m[:, 3] * v + m[:, 6], m[:, 1] * u + m[:, 4] * v + m[:, 7]
        d2 = d * d
        return (d2 < t2b * (lx * lx + ly * ly)) & (d2 < t2a * (kx * kx + ky * ky))


def update_num_iters(conf, w, s, max_iters):
    """OpenCV's RANSACUpdateNumIters(conf, 1 - w, s, max_iters) with the ceiling of the ratio"""
    conf, w = min(max(conf, 0.0), 1.0), min(max(w, 0.0), 1.0)
    ws = 1.0
    for _ in range(s):
        ws *= w
    num = math.log(max(1 - conf, np.finfo(np.float64).tiny))
    denom = 1 - ws
    if denom < np.finfo(np.float64).tiny:
        return 0
    denom = math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(math.ceil(num / denom))


def round_loop(n, s, slots, fin, seed, conf, max_iters, solve, key, smaller=False, shape=(3, 3)):
    """the sampling rounds of one pair, as every model and scoring runs them (csrc/ransac.h): ROUND hypotheses per round drawn by
    draw_samples; solve(idx [k, s]) -> (models [k, slots, *shape], number of models [k]) on the samples that were drawn and hold
    finite rows only; key(models [K, *shape]) -> (keys [K], inlier counts [K]): the inlier count itself, larger is better, or
    (smaller) a score, smaller is better, with the count carried along; the best key of the used slots (ties: lowest (h, slot))
    replaces the current model if it is strictly better; OpenCV's adaptive iteration count from the winner's inlier count;
    stop once ROUND * rounds reaches it or max_iters.
    Returns (best key, its inlier count, current model or None, best_h, best_root, rounds)."""
    worst = math.inf if smaller else -1
    best_key, best, cur, best_h, best_root, needed, rounds = worst, -1, None, -1, -1, max_iters, 0
    for r in range((max_iters + ROUND - 1) // ROUND):
        hs = np.arange(r * ROUND, (r + 1) * ROUND)
        idx, drawn = draw_samples(seed, hs, n, s)
        idx = np.where(drawn[:, None], idx, 0)
        ok = drawn & fin[idx].all(axis=1)
        models = np.zeros((ROUND, slots, *shape))
        nm = np.zeros(ROUND, dtype=np.int64)
        sel = np.nonzero(ok)[0]
        if len(sel):
            models[sel], nm[sel] = solve(idx[sel])
        keys, counts = key(models.reshape(-1, *shape))
        keys = np.where((np.arange(slots)[None, :] < nm[:, None]).reshape(-1), keys, worst)
        k = int(np.argmin(keys) if smaller else np.argmax(keys))  # the first one: lowest (h, slot)
        if keys[k] < best_key if smaller else keys[k] > best_key:
            best_key, best, best_h, best_root = keys[k].item(), int(counts[k]), r * ROUND + k // slots, k % slots
            cur = models.reshape(-1, *shape)[k].copy()
            needed = update_num_iters(conf, best / n, s, max_iters)
        rounds = r + 1
        if rounds * ROUND >= min(max_iters, needed):
            break
    return best_key, best, cur, best_h, best_root, rounds


def refit(model, xa, xb):
    """least-squares model on normalised inliers: smallest eigenvector of the 9 x 9 normal equations (rank 2 for F)"""
    x, y, u, v = xa[:, 0], xa[:, 1], xb[:, 0], xb[:, 1]
    one, zero = np.ones_like(x), np.zeros_like(x)
    if model == HOMOGRAPHY:
        A = np.concatenate([np.stack([x, y, one, zero, zero, zero, -u * x, -u * y, -u], 1),
                            np.stack([zero, zero, zero, x, y, one, -v * x, -v * y, -v], 1)])
    else:
        A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, one], 1)
    _, vec = np.linalg.eigh(A.T @ A)
    h = vec[:, 0].reshape(3, 3)
    if model == FUNDAMENTAL:
        U, S, Vt = np.linalg.svd(h)
        h = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    return h / np.linalg.norm(h)


def denormalise(model, cur, ca, sa, cb, sb):
    """the pixel model of a normalised one (H = Tb^-1 H_n Ta, F = Tb^T F_n Ta), scaled so that [2, 2] = 1"""
    Ta = np.array([[sa, 0, -sa * ca[0]], [0, sa, -sa * ca[1]], [0, 0, 1]])
    if model == HOMOGRAPHY:
        L = np.array([[1 / sb, 0, cb[0]], [0, 1 / sb, cb[1]], [0, 0, 1]])
    else:
        L = np.array([[sb, 0, 0], [0, sb, 0], [-sb * cb[0], -sb * cb[1], 1]])
    M = L @ cur @ Ta
    fro = np.linalg.norm(M)
    return M / (M[2, 2] if abs(M[2, 2]) >= 1e-12 * fro else fro)


def ransac(model, pa, pb, thr, conf, max_iters, seed, refine=True):
    """One pair.  pa, pb [n, 2] pixels (rows of the pair only).  Returns a dict: M [3, 3] (or zeros), mask [n], ok, rounds,
    best_h, best_root, best_min (count of the winning minimal-sample model), best (final count)."""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    n, s = len(pa), SAMPLE[model]
    out = dict(M=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), ok=False, rounds=0, best_h=-1, best_root=-1, best_min=-1, best=-1)
    if n < s:
        return out
    ca, sa, cb, sb, fin, cnt = normalize(pa, pb)
    if not (cnt >= s and math.isfinite(sa) and math.isfinite(sb)):
        return out
    with np.errstate(invalid="ignore"):
        xa, xb = (pa - ca) * sa, (pb - cb) * sb
    t2a, t2b = (thr * sa) ** 2, (thr * sb) ** 2

    def solve(idx):
        if model == HOMOGRAPHY:
            H, ok = solve_h(xa[idx], xb[idx])
            return H[:, None], ok.astype(np.int64)
        return solve_f(xa[idx], xb[idx])

    _, best, cur, best_h, best_root, rounds = round_loop(n, s, SLOTS[model], fin, seed, conf, max_iters, solve,
                                                         lambda M: (inliers(model, M, xa, xb, t2a, t2b).sum(axis=1),) * 2)
    out.update(rounds=rounds, best_h=best_h, best_root=best_root, best_min=best)
    if best <= 0:
        return out
    if refine:
        for _ in range(REFINE_ITERS):
            if best < REFIT_MIN[model]:
                break
            m = inliers(model, cur[None], xa, xb, t2a, t2b)[0]
            cand = refit(model, xa[m], xb[m])
            c = int(inliers(model, cand[None], xa, xb, t2a, t2b)[0].sum())
            if c < best:
                break
            best, cur = c, cand
    mask = inliers(model, cur[None], xa, xb, t2a, t2b)[0]
    M = denormalise(model, cur, ca, sa, cb, sb)
    out.update(M=M, mask=mask, ok=True, best=best)
    return out


def find_homography(pa, pb, ransac_reproj_threshold=3.0, confidence=0.995, max_iters=2000, seed=0, refine=True):
    """cv2.findHomography(pa, pb, RANSAC, ...) restated: (H [3, 3] or None, mask [n] or None)"""
    r = ransac(HOMOGRAPHY, pa, pb, ransac_reproj_threshold, confidence, max_iters, seed, refine)
    return (r["M"], r["mask"]) if r["ok"] else (None, None)


def find_fundamental(pa, pb, ransac_reproj_threshold=3.0, confidence=0.99, max_iters=1000, seed=0, refine=True):
    """cv2.findFundamentalMat(pa, pb, FM_RANSAC, ...) restated: (F [3, 3] or None, mask [n] or None)"""
    r = ransac(FUNDAMENTAL, pa, pb, ransac_reproj_threshold, confidence, max_iters, seed, refine)
    return (r["M"], r["mask"]) if r["ok"] else (None, None)
