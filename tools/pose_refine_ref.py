"""numpy float64 restatement of the device relative-pose refinement (roma_amd/csrc/pose_refine.hip `pose_refine_kernel`,
`roma_amd.refine_pose`, `estimate_pose(..., refine=True)`): the oracle of tests/test_gpu_pose_refine.py, as
tools/essential_ref.py is for the RANSAC and recoverPose it follows.

A Levenberg-Marquardt fit of (R, t) to the Sampson error under a hard-truncated loss - what the final refinement of
poselib.estimate_relative_pose is (the reference's romatch/benchmarks/megadepth_pose_estimation_benchmark_poselib.py).  PoseLib
is not a dependency and is not restated: the algorithm below is its own definition, shared step by step with the kernel.

State: rotation R, unit translation t, E = [t]x R, normalised points x0 = (x, y), x1 = (u, v).
  residual    p = R (x, y, 1), l = t x p (= E x0h), q = (u, v, 1) x t, k = R^T q (= E^T x1h),
              r = ((u l0 + v l1) + l2) / sqrt((l0^2 + l1^2) + (k0^2 + k1^2))
  parameters  R <- exp([w]x) R (Rodrigues), t <- normalise(t + d0 b0 + d1 b1) with the tangent basis of `tangent_basis`
  loop        cost, iteration and stopping rules are lm_ref.fit's, which tools/model_refine_ref.py shares; MIN_ROWS = 5; a
              threshold whose square is not finite is plain least squares over the finite rows there (the device call
              itself refuses thr = inf for the pose)
  mask        r^2 < thr^2 under the final pose and positive depth in both cameras (essential_ref.cheirality, distance DIST)
The device sums H, g and the cost in its own fixed order and calls its own sin / cos / sqrt: the two agree to rounding.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_ref as er  # noqa: E402
import lm_ref  # noqa: E402
from lm_ref import LAMBDA0, LAMBDA_MIN, PIVOT_REL, RETRIES, STEP_TOL, solve  # noqa: E402,F401

DIST = 1e9            # distance_thresh estimate_pose passes to recover_pose
MIN_ROWS = 5          # rows of a pair, and active rows of an iteration, below which nothing is fitted


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rodrigues(w):
    """exp([w]x) = I + a K + b K^2 with h = th / 2, s = sin(h) / h: a = sin(th) / th = s cos(h), b = (1 - cos(th)) / th^2 = s^2 / 2
    (no cancellation at small angles); a = 1, b = 1 / 2 for th^2 < 1e-30"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if th2 < 1e-30:
        a, b = 1.0, 0.5
    else:
        h = 0.5 * math.sqrt(th2)
        sh = math.sin(h) / h
        a, b = sh * math.cos(h), 0.5 * (sh * sh)
    K = skew(w)
    return np.eye(3) + a * K + b * (K @ K)


def tangent_basis(t):
    """b0 = normalise(t x e_a) with a the axis of the smallest |t_a| (first minimum), b1 = t x b0: [2, 3]"""
    a = int(np.argmin(np.abs(t)))
    e = np.zeros(3)
    e[a] = 1.0
    b0 = np.cross(t, e)
    b0 = b0 / math.sqrt((b0[0] * b0[0] + b0[1] * b0[1]) + b0[2] * b0[2])
    return np.stack([b0, np.cross(t, b0)])


def _parts(R, t, x0, x1):
    x, y, u, v = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    p = [(R[i, 0] * x + R[i, 1] * y) + R[i, 2] for i in range(3)]
    l = [t[1] * p[2] - t[2] * p[1], t[2] * p[0] - t[0] * p[2], t[0] * p[1] - t[1] * p[0]]
    q = [v * t[2] - t[1], t[0] - u * t[2], u * t[1] - v * t[0]]
    k = [(R[0, j] * q[0] + R[1, j] * q[1]) + R[2, j] * q[2] for j in range(2)]
    c = (u * l[0] + v * l[1]) + l[2]
    den = (l[0] * l[0] + l[1] * l[1]) + (k[0] * k[0] + k[1] * k[1])
    return p, l, q, k, c, den


def residuals(R, t, x0, x1):
    """signed Sampson distances [n] (NaN / inf where a row or the pose degenerates)"""
    with np.errstate(all="ignore"):
        _, _, _, _, c, den = _parts(R, t, x0, x1)
        return c / np.sqrt(den)


def jacobian(R, t, x0, x1):
    """(r [n], J [n, 5]): derivatives of r by (w0, w1, w2, d0, d1) at w = 0, d = 0"""
    with np.errstate(all="ignore"):
        u, v = x1[:, 0], x1[:, 1]
        p, l, q, k, c, den = _parts(R, t, x0, x1)
        s = np.sqrt(den)
        r = c / s
        inv_s, inv_den = 1.0 / s, 1.0 / den
        z, one = np.zeros_like(u), np.ones_like(u)
        bas = tangent_basis(t)
        # (dp, dq) of each parameter: rotation e_i x p and q x e_i (then through R^T); translation b x p and x1h x b
        dps = [(z, -p[2], p[1]), (p[2], z, -p[0]), (-p[1], p[0], z)]
        dqs = [(z, q[2], -q[1]), (-q[2], z, q[0]), (q[1], -q[0], z)]
        cols = []
        for i in range(5):
            if i < 3:
                dp = dps[i]
                dl = [t[1] * dp[2] - t[2] * dp[1], t[2] * dp[0] - t[0] * dp[2], t[0] * dp[1] - t[1] * dp[0]]
                dq = dqs[i]
            else:
                b = bas[i - 3]
                dl = [b[1] * p[2] - b[2] * p[1], b[2] * p[0] - b[0] * p[2], b[0] * p[1] - b[1] * p[0]]
                dq = [v * b[2] - b[1] * one, b[0] * one - u * b[2], u * b[1] - v * b[0]]
            dk = [(R[0, j] * dq[0] + R[1, j] * dq[1]) + R[2, j] * dq[2] for j in range(2)]
            dc = (u * dl[0] + v * dl[1]) + dl[2]
            cols.append(dc * inv_s - r * (((l[0] * dl[0] + l[1] * dl[1]) + (k[0] * dk[0] + k[1] * dk[1])) * inv_den))
        return r, np.stack(cols, axis=1)


def active(r, thr):
    with np.errstate(invalid="ignore"):
        return np.isfinite(r) & (r * r < thr * thr)


def cost(R, t, x0, x1, thr):
    """(truncated cost, active rows)"""
    c, a = lm_ref.truncated(residuals(R, t, x0, x1)[:, None], thr)
    return c, int(a.sum())


def apply(R, t, delta):
    """the pose after the step delta = (w, d)"""
    bas = tangent_basis(t)
    t1 = (t + delta[3] * bas[0]) + delta[4] * bas[1]
    t1 = t1 / math.sqrt((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2])
    return rodrigues(delta[:3]) @ R, t1


class PoseFit:
    """the problem as lm_ref.fit takes it: state (R, t), rows (x0, x1)"""
    MIN_ROWS = MIN_ROWS

    @staticmethod
    def jacobian(st, w):
        r, J = jacobian(st[0], st[1], w[0], w[1])
        return r[:, None], J

    @staticmethod
    def normal(J, e, a):
        return J[a].T @ J[a], J[a].T @ e[a, 0]

    @staticmethod
    def residuals(st, w):
        return residuals(st[0], st[1], w[0], w[1])[:, None]

    @staticmethod
    def apply(st, d):
        return apply(st[0], st[1], d)


def refine(R, t, x0, x1, thr, max_steps=25, valid=True):
    """One pair on normalised points [n, 2] (what the device reads, i.e. f32-rounded).  Returns a dict: R [3, 3], t [3],
    mask [n], info = (accepted steps, cost evaluations, active rows at the end, pair valid), cost0, cost."""
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64).reshape(3)
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    n = len(x0)
    tn = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    ok = bool(valid) and n >= MIN_ROWS and np.isfinite(R).all() and np.isfinite(t).all() and tn > 0 and thr > 0
    out = dict(R=R, t=t, mask=np.zeros(n, dtype=bool), info=(0, 0, 0, int(ok)), cost0=math.nan, cost=math.nan)
    if not ok:
        return out
    (Rc, tc), steps, evals, a, cost0, cur = lm_ref.fit(PoseFit, (R, t / tn), (x0, x1), thr, max_steps)
    with np.errstate(all="ignore"):
        mask = a & er.cheirality(Rc, tc, x0, x1, DIST)
    # without an accepted step the input comes back untouched, whatever the norm of its t
    out.update(R=Rc, t=tc if steps else t, mask=mask, info=(steps, evals, int(a.sum()), 1), cost0=cost0, cost=cur)
    return out


def normalise(kpts0, kpts1, K0, K1):
    """the normalised points of essential_ref.estimate_pose, rounded to f32 as the device reads them"""
    K0inv, K1inv = np.linalg.inv(K0[:2, :2]), np.linalg.inv(K1[:2, :2])
    x0 = (K0inv @ (np.asarray(kpts0, dtype=np.float64) - K0[None, :2, 2]).T).T.astype(np.float32).astype(np.float64)
    x1 = (K1inv @ (np.asarray(kpts1, dtype=np.float64) - K1[None, :2, 2]).T).T.astype(np.float32).astype(np.float64)
    return x0, x1


def refine_pose(R, t, kpts0, kpts1, K0, K1, norm_thresh, max_steps=25):
    """roma_amd.refine_pose for one pair of pixel keypoints: (R, t [3, 1], mask, info)"""
    x0, x1 = normalise(kpts0, kpts1, K0, K1)
    o = refine(R, np.asarray(t).reshape(3), x0, x1, norm_thresh, max_steps)
    return o["R"], o["t"][:, None].copy(), o["mask"], o["info"]


def estimate_pose(kpts0, kpts1, K0, K1, norm_thresh, conf=0.99999, max_iters=1000, seed=0, max_steps=25):
    """essential_ref.estimate_pose followed by the refinement, as roma_amd.estimate_pose(..., refine=True): (R, t [3, 1], mask)
    or None"""
    got = er.estimate_pose(kpts0, kpts1, K0, K1, norm_thresh, conf, max_iters, seed)
    if got is None:
        return None
    R, t, mask, _ = refine_pose(got[0], got[1], kpts0, kpts1, K0, K1, norm_thresh, max_steps)
    return R, t, mask
