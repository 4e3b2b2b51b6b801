"""Scenes of the registration tests (test_cpu_registration.py, test_gpu_registration.py): the 3-D points of the relief scene of
absolute_pose_cases.scene as the source, dst = s R x + t plus Gaussian noise, an outlier's destination uniform in the
destination's bounding box and at least 10 thresholds from the true point; exact, random and collinear three-point samples; a
planar set; the ragged batch; SVD Umeyama as the independent route.  Everything the device sees goes through f32 first."""
import functools
import math
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import registration_ref as rr  # noqa: E402
from absolute_pose_cases import scene as relief_scene  # noqa: E402

THR_REL = 0.02     # threshold of the scenes over the scale: 0.02 in the source's units (the relief spans about 4)
NOISE_REL = 0.15   # noise per coordinate over the threshold: |noise| < thr is a 6.7 sigma event, every true inlier is inside
SCALES = (0.37, 1.0, 2.9)
SHIFT = (1e3, -2e3, 5e2)
MIN_TRIANGLE = 0.2  # |d12 x d13| / (|d12| |d13|) of the exact and random samples: far from the collinear refusal at 1e-4


def f32(x):  # what the device sees
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def rotation(g, max_angle=math.pi):
    """a rotation about a random axis by an angle uniform in [0, max_angle]"""
    ax = g.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = g.uniform(0, max_angle)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * (Kx @ Kx)


def triangle_ratio(p):
    """|d12 x d13| / (|d12| |d13|) of p [M, 3, 3]"""
    d12, d13 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return np.linalg.norm(np.cross(d12, d13), axis=1) / (np.linalg.norm(d12, axis=1) * np.linalg.norm(d13, axis=1))


@functools.lru_cache(maxsize=None)
def scene(n=2000, outlier_frac=0.3, scale=1.0, rng_seed=1, shift=False, rigid_noise=True):
    """(X [n, 3], Y [n, 3] as the device sees them, true inliers [n], (s, R, t), thr)"""
    X = relief_scene(n=n, outlier_frac=0.0, rng_seed=rng_seed)[3]
    g = np.random.default_rng(1000 + rng_seed)
    R, t = rotation(g), g.uniform(-3, 3, 3)
    thr = THR_REL * scale
    true = scale * X @ R.T + t
    Y = true + NOISE_REL * thr * g.normal(size=true.shape)
    out = g.random(n) < outlier_frac
    lo, hi = true.min(axis=0), true.max(axis=0)
    for i in np.nonzero(out)[0]:
        while True:
            c = g.uniform(lo, hi)
            if np.linalg.norm(c - true[i]) > 10 * thr:
                Y[i] = c
                break
    if shift:  # both sets moved: y + d = s R (x + d) + (t + d - s R d)
        d = np.asarray(SHIFT)
        X, Y, t = X + d, Y + d, t + d - scale * R @ d
    return f32(X), f32(Y), ~out, (scale, R, t), thr


# the scenes of the RANSAC agreement test: (outlier share, seed, scale, shifted origin)
AGREEMENT = [(frac, seed, s, False) for frac in (0.3, 0.5) for seed in (1, 2, 3) for s in SCALES] + [(0.3, 1, 2.9, True), (0.5, 2, 0.37, True)]
REFINE_SEEDS = (0, 1, 2, 3)


def agreement_scene(frac, seed, s, shift):
    return scene(2000, frac, s, rng_seed=seed, shift=shift)


def model_error(s, R, t, s0, R0, t0):
    """max(|dR|_max, |ds| / s0, |dt|_max / max(1, |t0|_max)) over the trailing axes"""
    return np.maximum(np.maximum(np.abs(R - R0).max(axis=(-2, -1)), np.abs(s - s0) / s0),
                      np.abs(t - t0).max(axis=-1) / np.maximum(1.0, np.abs(t0).max(axis=-1)))


def _triangles(g, m):
    X = np.zeros((0, 3, 3))
    while len(X) < m:
        c = g.uniform(-2, 2, (2 * m, 3, 3))
        X = np.concatenate([X, c[triangle_ratio(c) >= MIN_TRIANGLE]])
    return X[:m]


def exact_samples(m, seed):
    """(X, Y [m, 3, 3], s [m], R [m, 3, 3], t [m, 3]): triangles of ratio >= MIN_TRIANGLE, Y = s R X + t exactly (to f64 rounding),
    s log-uniform in [0.2, 5], t uniform in [-3, 3]^3"""
    g = np.random.default_rng(seed)
    X = _triangles(g, m)
    s = np.exp(g.uniform(math.log(0.2), math.log(5.0), m))
    R = np.stack([rotation(g) for _ in range(m)])
    t = g.uniform(-3, 3, (m, 3))
    Y = s[:, None, None] * np.einsum("mij,mkj->mki", R, X) + t[:, None]
    return X, Y, s, R, t


def random_samples(m, seed):
    """(X, Y [m, 3, 3]): two unrelated triangles of ratio >= MIN_TRIANGLE each - no similarity fits them, the closed form gives the
    least-squares one"""
    g = np.random.default_rng(seed)
    return _triangles(g, m), 3.0 * _triangles(g, m) + g.uniform(-5, 5, (m, 1, 3))


def collinear_samples(m, seed):
    """(X, Y [m, 3, 3]): the source's three points on a line in the first half, the destination's in the second"""
    g = np.random.default_rng(seed)
    X, Y, *_ = exact_samples(m, seed)
    line = g.uniform(-2, 2, (m, 1, 3)) + g.uniform(-1, 1, (m, 1, 3)) * np.array([0.0, 1.0, 2.5])[None, :, None]
    X[:m // 2], Y[m // 2:] = line[:m // 2], line[m // 2:]
    return X, Y


def planar_scene(n=500, seed=7, scale=1.7):
    """a planar source (z = 0.25 everywhere): rank-2 moments, which the closed form must handle"""
    g = np.random.default_rng(seed)
    X = np.c_[g.uniform(-2, 2, (n, 2)), np.full(n, 0.25)]
    R, t = rotation(g), g.uniform(-3, 3, 3)
    return f32(X), f32(scale * X @ R.T + t), (scale, R, t)


def umeyama_svd(X, Y, with_scale=True):
    """the independent route: Umeyama (1991) through numpy.linalg.svd, det R = +1"""
    xb, yb = X.mean(axis=0), Y.mean(axis=0)
    dx, dy = X - xb, Y - yb
    U, D, Vt = np.linalg.svd(dy.T @ dx)
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    s = float((D * np.diag(S)).sum() / (dx * dx).sum()) if with_scale else 1.0
    return s, R, yb - s * R @ xb


RAGGED_COUNTS = [0, 3, 4, 63, 65, 257]


def ragged_batch(fill):
    """B = 6 problems of N = 257 rows with counts (0, 3, 4, 63, 65, 257); rows beyond counts[b] hold `fill`; the first four rows of
    every problem are inliers"""
    Xs, Ys = np.full((6, 257, 3), fill), np.full((6, 257, 3), fill)
    thr = None
    for b, c in enumerate(RAGGED_COUNTS):
        X, Y, truth, _, thr = scene(257, 0.2, 1.0, rng_seed=20 + b)
        order = np.r_[np.nonzero(truth)[0][:4], np.setdiff1d(np.arange(257), np.nonzero(truth)[0][:4])]
        Xs[b, :c], Ys[b, :c] = X[order][:c], Y[order][:c]
    return Xs, Ys, thr


def residual(model, X, Y):
    """|s R x + t - y| per row"""
    s, R, t = model
    return np.linalg.norm(s * X @ np.asarray(R).T + np.asarray(t).reshape(3) - Y, axis=1)


# ---- depth maps and trajectories
def depth_case(H=37, W=53, seed=5):
    """two depth maps of one view in gauges that differ by a known similarity: reconstruction a holds the view at pose (Ra, ta)
    with depth d; reconstruction b = the similarity (s, R, t)^-1 of a, so b -> a is (s, R, t): X_a = s R X_b + t.  The camera of b:
    R_b = R_a R, t_b = (R_a t + t_a) / s, depth_b = depth_a / s.  NaN, zero and negative depths sprinkled into both maps."""
    g = np.random.default_rng(seed)
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1.0]])
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    da = 4.0 + 0.6 * np.sin(xs / W * 5.0 + 1.0) + 0.4 * np.cos(ys / H * 4.0 + 2.0)
    s, R, t = 2.3, rotation(g), g.uniform(-3, 3, 3)
    Ra, ta = rotation(g, 0.3), g.uniform(-1, 1, 3)
    Rb, tb = Ra @ R, (Ra @ t + ta) / s
    da32, db32 = da.astype(np.float32), (da / s).astype(np.float32)
    for d in (da32, db32):
        bad = g.integers(0, H * W, 40)
        d.reshape(-1)[bad[:14]] = np.nan
        d.reshape(-1)[bad[14:27]] = 0.0
        d.reshape(-1)[bad[27:]] = -1.0
    return dict(K=K, da=da32, db=db32, Ra=Ra, ta=ta, Rb=Rb, tb=tb, sim=(s, R, t))


def trajectory_case(V, seed, noise=0.01, collinear=False):
    """a true path of V cameras, and the recovered one: the true one in another gauge (X_gt = s R X + t) with noise on the centres
    and a small rotation error per view: (R, t, R_gt, t_gt, (s, R_sim, t_sim))"""
    g = np.random.default_rng(seed)
    Rg = np.stack([rotation(g, 0.5) for _ in range(V)])
    cg = g.uniform(-2, 2, (V, 3)) if not collinear else np.linspace(0, 1, V)[:, None] * np.array([1.0, 2.0, -0.5]) + 0.3
    tg = -np.einsum("vij,vj->vi", Rg, cg)
    s, Rs, ts = 1.8, rotation(g), g.uniform(-3, 3, 3)
    # the recovered gauge: X = (s Rs)^-1 (X_gt - ts); camera R_c = R_gt Rs, centre c = Rs^T (c_gt - ts) / s
    c = (cg - ts) @ Rs / s + (noise * g.normal(size=(V, 3)) if not collinear else 0.0)
    R = np.stack([rotation(g, 0.01) @ Rg[v] @ Rs for v in range(V)])
    t = -np.einsum("vij,vj->vi", R, c)
    return R, t, Rg, tg, (s, Rs, ts)
