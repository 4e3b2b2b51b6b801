"""Scenes of the bundle adjustment for its tests (tests/bundle_cases.py) and its microbenchmark (tools/bench_bundle.py): points
on the relief of accuracy_harness.synthetic_relief_pair (depth 3 - 5) seen by V cameras.  View 0 is the identity; every further
view is rotated by 0.05 - 0.25 rad about a random axis with its centre 0.4 - 0.7 away, a third to two thirds of that along the
optical axis: with a purely lateral baseline the held translation component says little about the scale and the fit crawls."""
import numpy as np

from bundle_ref import rodrigues


def relief_depth(px, py, h, w, ph):
    """the relief of synthetic_relief_pair (depth 3 .. 5) at pixel coordinates"""
    return 4.0 + 0.6 * np.sin(px / w * 5.0 + ph[0]) + 0.4 * np.cos(py / h * 4.0 + ph[1])


H, W = 480, 640
K0 = np.array([[520.0, 0.0, 320.0], [0.0, 515.0, 240.0], [0.0, 0.0, 1.0]])


def project(K, R, t, X):
    """pixels [V, n, 2] and depths [V, n] of the points in every view"""
    p = np.einsum("vij,nj->vni", R, X) + t[:, None]
    return np.stack([K[:, 0, 0, None] * p[..., 0] / p[..., 2] + K[:, 0, 2, None], K[:, 1, 1, None] * p[..., 1] / p[..., 2] + K[:, 1, 2, None]], 2), p[..., 2]


def scene(V, n, seed, missing=0.0, noise_px=0.0, outlier_frac=0.0, thr=2.0):
    """dict: K [V, 3, 3], R [V, 3, 3], t [V, 3], X [n, 3], kpts [V, n, 2] (NaN where not observed), truth [V, n]: observed and no
    outlier.  An outlier's pixel is uniform in the image and at least 10 thr from the true projection."""
    g = np.random.default_rng(seed)
    K = np.stack([K0 * [[1 + 0.02 * i], [1 - 0.01 * i], [1]] for i in range(V)])
    R, t = [np.eye(3)], [np.zeros(3)]
    for _ in range(1, V):
        ax = g.normal(size=3)
        Ri = rodrigues(ax / np.linalg.norm(ax) * g.uniform(0.05, 0.25))
        d, fwd = g.uniform(0.4, 0.7), g.uniform(1 / 3, 2 / 3) * g.choice([-1.0, 1.0])
        lat = g.normal(size=2)
        C = d * np.r_[np.sqrt(1 - fwd * fwd) * lat / np.linalg.norm(lat), fwd]
        R.append(Ri)
        t.append(-Ri @ C)
    R, t = np.stack(R), np.stack(t)
    ph = g.uniform(0, 6, 2)
    pa = g.uniform([0, 0], [W, H], (n, 2))
    X = np.c_[(pa[:, 0] - K[0, 0, 2]) / K[0, 0, 0], (pa[:, 1] - K[0, 1, 2]) / K[0, 1, 1], np.ones(n)] * relief_depth(pa[:, 0], pa[:, 1], H, W, ph)[:, None]
    true, z = project(K, R, t, X)
    assert (z > 1).all()
    kp = true + noise_px * g.normal(size=true.shape)
    out = g.random((V, n)) < outlier_frac
    for i, j in zip(*np.nonzero(out)):
        while True:
            c = g.uniform([0, 0], [W, H])
            if np.linalg.norm(c - true[i, j]) > 10 * thr:
                kp[i, j] = c
                break
    gone = g.random((V, n)) < missing
    kp[gone] = np.nan
    return dict(K=K, R=R, t=t, X=X, kpts=kp, truth=~out & ~gone)


def start(s, seed, dX=1e-2, dpose=3e-3):
    """a start near the scene: points moved by dX, every pose but view 0's by dpose (rotation vector and translation)"""
    g = np.random.default_rng(seed)
    R, t = s["R"].copy(), s["t"].copy()
    for i in range(1, len(R)):
        R[i] = rodrigues(dpose * g.normal(size=3)) @ R[i]
        t[i] = t[i] + dpose * g.normal(size=3)
    return s["X"] + dX * g.normal(size=s["X"].shape), R, t
