"""numpy float64 restatement of roma_op_warp_kpts and roma_op_dense_metrics (csrc/gt_warp.hip; the definition is in
include/roma_hip.h) - the oracle of tests/test_gpu_gt_warp.py, itself checked against recorded outputs of the reference's
warp_kpts / get_gt_warp / geometric_dist by tests/test_cpu_gt_warp.py.  Every expression below is written with elementwise
+ - * / floor sqrt in the order the kernel uses (no matrix product and no matrix inverse, whose order of operations numpy does not
fix), so both sides round alike."""
from __future__ import annotations

import numpy as np

EDGE = 1e-9  # a quantity this close (relative) to a threshold it is tested against may fall either way on the device


def _near(q, thr):
    """rows whose quantity lies within EDGE relative of the threshold (absolute for a threshold of 0)"""
    with np.errstate(invalid="ignore"):
        return np.abs(q - thr) <= EDGE * (abs(thr) if thr != 0 else 1.0)


def inverse3(K):
    """adjugate / determinant of a general 3 x 3, in the kernel's order"""
    a, b, c, d, e, f, g, h, i = np.asarray(K, dtype=np.float64).reshape(9)
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = (a * c00 + b * c10) + c * c20
    with np.errstate(all="ignore"):
        return np.array([[c00 / det, c01 / det, c02 / det], [c10 / det, c11 / det, c12 / det], [c20 / det, c21 / det, c22 / det]])


def sample(D, x, y):
    """torch grid_sample (bilinear, align_corners=False, zeros padding) of one map D [Hs, Ws] (float32) at normalised x, y [L] in
    float64: in and out of range is decided in float64, a tap out of range contributes 0, a non-finite coordinate samples 0"""
    D = np.asarray(D)
    Hs, Ws = D.shape
    Dd = D.astype(np.float64)
    with np.errstate(all="ignore"):
        ix, iy = ((x + 1.0) * float(Ws) - 1.0) / 2.0, ((y + 1.0) * float(Hs) - 1.0) / 2.0
        x0, y0 = np.floor(ix), np.floor(iy)
        x1, y1 = x0 + 1.0, y0 + 1.0
        wx0, wx1, wy0, wy1 = x1 - ix, ix - x0, y1 - iy, iy - y0
        xm, ym = float(Ws - 1), float(Hs - 1)
        w_in, e_in = (x0 >= 0.0) & (x0 <= xm), (x1 >= 0.0) & (x1 <= xm)
        n_in, s_in = (y0 >= 0.0) & (y0 <= ym), (y1 >= 0.0) & (y1 <= ym)

        def tap(ok, yy, xx, wgt):
            yi, xi = np.where(ok, yy, 0.0).astype(np.int64), np.where(ok, xx, 0.0).astype(np.int64)
            return np.where(ok, Dd[yi, xi] * wgt, 0.0)
        acc = tap(n_in & w_in, y0, x0, wx0 * wy0)
        acc = acc + tap(n_in & e_in, y0, x1, wx1 * wy0)
        acc = acc + tap(s_in & w_in, y1, x0, wx0 * wy1)
        acc = acc + tap(s_in & e_in, y1, x1, wx1 * wy1)
    return acc


def grid_axis(n):
    """the n pixel centres of [-1, 1] as the kernel generates them: (2 j + 1) / n - 1 in float64, rounded once to float32"""
    j = np.arange(n, dtype=np.float64)
    return ((2.0 * j + 1.0) / float(n) - 1.0).astype(np.float32)


def grid(H, W):
    """[H * W, 2] float32 (x, y) key points of get_gt_warp, row-major"""
    gx, gy = np.meshgrid(grid_axis(W), grid_axis(H))
    return np.stack([gx, gy], axis=-1).reshape(H * W, 2)


def warp_kpts(kpts0, depth0, depth1, T_0to1, K0, K1, relative_depth_error_threshold=0.05):
    """ONE pair: kpts0 [L, 2] normalised (float32 or float64, widened exactly), depth0 [H0, W0], depth1 [H1, W1] float32, T [3, 4] or
    [4, 4], K0, K1 [3, 3].  Returns a dict: valid bool [L], warped [L, 2], rel [L], and the parts nonzero, covisible, consistent,
    u, v (pixels of image 1) and near bool [L] (a deciding quantity within EDGE of its threshold)."""
    k = np.asarray(kpts0).astype(np.float64)
    x, y = k[:, 0], k[:, 1]
    H0, W0 = np.asarray(depth0).shape
    H1, W1 = np.asarray(depth1).shape
    T, K1 = np.asarray(T_0to1, dtype=np.float64), np.asarray(K1, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    Ki = inverse3(K0)
    thr = float(relative_depth_error_threshold)
    with np.errstate(all="ignore"):
        px, py = float(W0) * (x + 1.0) / 2.0, float(H0) * (y + 1.0) / 2.0
        d0 = sample(depth0, x, y)
        nonzero = d0 != 0.0
        h0, h1, h2 = px * d0, py * d0, d0
        X = [(Ki[i, 0] * h0 + Ki[i, 1] * h1) + Ki[i, 2] * h2 for i in range(3)]
        Y = [((R[i, 0] * X[0] + R[i, 1] * X[1]) + R[i, 2] * X[2]) + t[i] for i in range(3)]
        P = [(K1[i, 0] * Y[0] + K1[i, 1] * Y[1]) + K1[i, 2] * Y[2] for i in range(3)]
        den = P[2] + 1e-4
        u, v = P[0] / den, P[1] / den
        covisible = (u > 0.0) & (u < float(W1 - 1)) & (v > 0.0) & (v < float(H1 - 1))
        wx, wy = 2.0 * u / float(W1) - 1.0, 2.0 * v / float(H1) - 1.0
        d1 = sample(depth1, wx, wy)
        rel = np.abs((d1 - Y[2]) / d1)
        consistent = rel < thr
    near = _near(u, 0.0) | _near(u, float(W1 - 1)) | _near(v, 0.0) | _near(v, float(H1 - 1)) | _near(rel, thr)
    return {"valid": nonzero & covisible & consistent, "warped": np.stack([wx, wy], axis=-1), "rel": rel, "nonzero": nonzero,
            "covisible": covisible, "consistent": consistent, "u": u, "v": v, "near": near}


def get_gt_warp(depth1, depth2, T_1to2, K1, K2, relative_depth_error_threshold=0.05, H=None, W=None):
    """ONE pair: (x2 [H, W, 2] float64, prob [H, W] float32, near [H, W])"""
    if H is None:
        H, W = np.asarray(depth1).shape
    o = warp_kpts(grid(H, W), depth1, depth2, T_1to2, K1, K2, relative_depth_error_threshold)
    return o["warped"].reshape(H, W, 2), o["valid"].astype(np.float32).reshape(H, W), o["near"].reshape(H, W)


def dense_metrics(dense_matches, depth1, depth2, T_1to2, K1, K2, relative_depth_error_threshold=0.05, thresholds=(1.0, 3.0, 5.0)):
    """ONE pair: dense_matches [h, w, 4] float32.  Returns a dict: prob float32 [h, w], gd float64 [h, w] (every pixel: mask it with
    prob), n_valid, n_below [3], gd_sum (ascending index) and near bool [h, w]."""
    m = np.asarray(dense_matches)
    assert m.dtype == np.float32 and m.ndim == 3 and m.shape[2] == 4
    h, w = m.shape[:2]
    o = warp_kpts(m[..., :2].reshape(-1, 2), depth1, depth2, T_1to2, K1, K2, relative_depth_error_threshold)
    one, two = np.float32(1.0), np.float32(2.0)
    xh = (np.float32(w) * (m[..., 2].reshape(-1) + one)) / two  # float32, as the reference forms it
    yh = (np.float32(h) * (m[..., 3].reshape(-1) + one)) / two
    assert xh.dtype == np.float32
    with np.errstate(all="ignore"):
        tx, ty = float(w) * (o["warped"][:, 0] + 1.0) / 2.0, float(h) * (o["warped"][:, 1] + 1.0) / 2.0
        dx, dy = xh.astype(np.float64) - tx, yh.astype(np.float64) - ty
        gd = np.sqrt(dx * dx + dy * dy)
    valid = o["valid"]
    near = o["near"].copy()
    for thr in thresholds:
        near |= valid & _near(gd, float(thr))
    gd_sum = 0.0
    for g in gd[valid]:
        gd_sum = gd_sum + float(g)
    return {"prob": valid.astype(np.float32).reshape(h, w), "gd": gd.reshape(h, w), "n_valid": int(valid.sum()),
            "n_below": np.array([int((gd[valid] < float(thr)).sum()) for thr in thresholds], dtype=np.int64), "gd_sum": gd_sum,
            "near": near.reshape(h, w), "warped": o["warped"].reshape(h, w, 2)}
