"""Scenes of the absolute-pose tests (test_cpu_absolute_pose.py, test_gpu_absolute_pose.py): exact P3P samples and the relief
scene of tools/accuracy_harness.synthetic_relief_pair - its K, R, t and a relief depth of 3 - 5 - with the 3-D points, a noise
level and an outlier share placed at least 10 thresholds from the true projection."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import absolute_pose_ref as ar  # noqa: E402
from accuracy_harness import synthetic_relief_pair  # noqa: E402

THR = 1.0  # reprojection threshold of the scenes, pixels


def f32(x):  # what the device sees
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def exact_samples(m, seed):
    """(X [m, 3, 3], x [m, 3, 2], R [m, 3, 3], t [m, 3]): random axis, angle uniform in [0, 1] rad, three camera-frame points with
    normalised image coordinates uniform in [-0.6, 0.6]^2 and depths uniform in [2, 10], t uniform in [-1, 1]^3, X = R^T (Y - t)"""
    g = np.random.default_rng(seed)
    ax = g.normal(size=(m, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = g.uniform(0, 1, m)
    R = np.stack([ar.rodrigues(a * w) for a, w in zip(ax, ang)])
    x = g.uniform(-0.6, 0.6, (m, 3, 2))
    d = g.uniform(2, 10, (m, 3))
    Y = np.concatenate([x, np.ones((m, 3, 1))], 2) * d[..., None]
    t = g.uniform(-1, 1, (m, 3))
    X = np.einsum("mji,mkj->mki", R, Y - t[:, None])
    return X, x, R, t


def pose_error(R, t, R0, t0):
    """max(|dR|_max, |dt|_max / max(1, |t0|_max)) over the trailing axes"""
    return np.maximum(np.abs(R - R0).max(axis=(-2, -1)), np.abs(t - t0).max(axis=-1) / np.maximum(1.0, np.abs(t0).max(axis=-1)))


def true_pose_error(Rs, ts, n, R, t):
    """per sample, the smallest pose_error of its solutions against the true pose (inf without a solution)"""
    err = np.full(len(n), np.inf)
    for s in range(Rs.shape[1]):
        err = np.where(s < n, np.minimum(err, pose_error(Rs[:, s], ts[:, s], R, t)), err)
    return err


def relief_depth(px, py, h, w, ph):
    """the relief of synthetic_relief_pair (depth 3 .. 5) at pixel coordinates"""
    return 4.0 + 0.6 * np.sin(px / w * 5.0 + ph[0]) + 0.4 * np.cos(py / h * 4.0 + ph[1])


def scene(n=2000, outlier_frac=0.3, noise_px=0.0, seed=3, rng_seed=1, h=480, w=640, thr=THR, shift=(0.0, 0.0, 0.0)):
    """(K, R, t, X [n, 3], kpts [n, 2], inlier truth): points of the relief seen from camera A (the world frame, moved by `shift`),
    their exact pixels in camera B (plus noise_px of Gaussian noise); an outlier's pixel is uniform in the image and at least
    10 thr from the true projection.  x_B ~ K (R X + t)."""
    d = synthetic_relief_pair(h, w, seed=seed)
    K, T = d["K1"], d["T_1to2"]
    U, _, Vt = np.linalg.svd(T[:, :3])  # the pair's R comes from f32 sin / cos: orthonormal to 1e-8 only
    R, t = U @ Vt, T[:, 3].copy()
    rng = np.random.default_rng(rng_seed)
    ph = rng.uniform(0, 6, 2)
    X, kp = np.zeros((0, 3)), np.zeros((0, 2))
    while len(X) < n:
        pa = rng.uniform([0, 0], [w, h], (2 * n, 2))
        Y = np.c_[(pa[:, 0] - K[0, 2]) / K[0, 0], (pa[:, 1] - K[1, 2]) / K[1, 1], np.ones(2 * n)] * relief_depth(pa[:, 0], pa[:, 1], h, w, ph)[:, None]
        q = Y @ R.T + t
        pb = np.stack([K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2], K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]], 1)
        vis = (q[:, 2] > 0) & (pb[:, 0] > 0) & (pb[:, 0] < w) & (pb[:, 1] > 0) & (pb[:, 1] < h)
        X, kp = np.concatenate([X, Y[vis]]), np.concatenate([kp, pb[vis]])
    X, kp = X[:n], kp[:n]
    true = kp.copy()
    kp = kp + noise_px * rng.normal(size=kp.shape)
    out = rng.random(n) < outlier_frac
    for i in np.nonzero(out)[0]:
        while True:
            c = rng.uniform([0, 0], [w, h])
            if np.linalg.norm(c - true[i]) > 10 * thr:
                kp[i] = c
                break
    shift = np.asarray(shift, dtype=np.float64)
    # the world frame moved by shift: X_w = X + shift, x_cam = R (X_w - shift) + t
    return K, R, t - R @ shift, X + shift, kp, ~out


def reproj2(R, t, X, kp, K):
    """squared reprojection error in normalised image coordinates (inf behind the camera), and the normalised threshold scale"""
    q = X @ R.T + t
    with np.errstate(all="ignore"):
        e = np.stack([q[:, 0] / q[:, 2] - (kp[:, 0] - K[0, 2]) / K[0, 0], q[:, 1] / q[:, 2] - (kp[:, 1] - K[1, 2]) / K[1, 1]], 1)
        return np.where(q[:, 2] > 0, (e * e).sum(1), np.inf)


def rot_angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))
