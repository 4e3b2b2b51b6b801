"""numpy float64 restatement of roma_op_triangulate and roma_op_depth_consistency (csrc/triangulate.hip; the definition is in
include/roma_hip.h) - the oracle of tests/test_gpu_triangulate.py.  Every expression below is written with elementwise + - * /
sqrt in the order the kernel uses (no matrix product, whose summation order numpy does not fix), so both sides round alike and
differ only in atan2's last bits and in the final rounding to float32.

One-sided error model: the pixel on the grid of the reference image is exact, the predicted coordinate in the other image
carries the error; the point lies on the reference pixel's ray at the depth whose projection into the other image is closest
to the prediction, i.e. at the foot of the prediction on the ray's epipolar line."""
from __future__ import annotations

import numpy as np

SKIPPED, DEGENERATE, CHEIRALITY, REPROJ, PARALLAX, CERTAINTY = 1, 2, 4, 8, 16, 32
RAD_TO_DEG = 57.29577951308232  # 180 / pi, the kernel's constant
EDGE = 1e-9  # a quantity this close (relative) to a threshold it is tested against may fall either way on the device


def _cam(K):
    """(fx, fy, cx, cy) of a [3, 3] matrix, identity for None"""
    if K is None:
        return 1.0, 1.0, 0.0, 0.0
    K = np.asarray(K, dtype=np.float64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def inverse_pose(R, t):
    """(R^T, -R^T t) in the kernel's order of operations"""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3)
    ti = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])
    return R.T.copy(), ti


def _near(q, thr):
    """rows whose quantity lies within EDGE relative of the threshold"""
    if not np.isfinite(thr):
        return np.zeros(q.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.abs(q - thr) <= EDGE * abs(thr)


def triangulate_view(ref, obs, R, t, K_r, K_o, certainty=None, max_depth=np.inf, max_reproj=np.inf, min_parallax=0.0,
                     min_certainty=0.0):
    """One view of one pair: ref [m, 2] reference pixels (exact), obs [m, 2] observed pixels in the other image, (R, t) mapping
    reference-frame points to the other frame.  Returns a dict of float64 arrays: points [m, 3], depth_other, reproj, parallax
    [m], flags uint8 [m] (bits DEGENERATE .. CERTAINTY) and near [m] bool (threshold edges).  Degenerate rows hold NaN."""
    ref, obs = np.asarray(ref, dtype=np.float64), np.asarray(obs, dtype=np.float64)
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3)
    fxr, fyr, cxr, cyr = _cam(K_r)
    fxo, fyo, cxo, cyo = _cam(K_o)
    u, v, uo, vo = ref[:, 0], ref[:, 1], obs[:, 0], obs[:, 1]
    pose_ok = bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and np.all(np.isfinite([fxr, fyr, cxr, cyr, fxo, fyo, cxo, cyo])))
    finite_in = np.isfinite(u) & np.isfinite(v) & np.isfinite(uo) & np.isfinite(vo)
    with np.errstate(all="ignore"):
        x0, x1 = (u - cxr) / fxr, (v - cyr) / fyr
        r0 = (R[0, 0] * x0 + R[0, 1] * x1) + R[0, 2]
        r1 = (R[1, 0] * x0 + R[1, 1] * x1) + R[1, 2]
        r2 = (R[2, 0] * x0 + R[2, 1] * x1) + R[2, 2]
        A0, A1, A2 = fxo * r0 + cxo * r2, fyo * r1 + cyo * r2, r2
        bv0, bv1, bv2 = fxo * t[0] + cxo * t[2], fyo * t[1] + cyo * t[2], t[2]
        l0, l1, l2 = A1 * bv2 - A2 * bv1, A2 * bv0 - A0 * bv2, A0 * bv1 - A1 * bv0
        n2 = l0 * l0 + l1 * l1
        degenerate = ~(pose_ok & finite_in & (n2 > 0.0))
        s = (l0 * uo + l1 * vo) + l2
        d = s / np.sqrt(n2)
        px, py = uo - (s * l0) / n2, vo - (s * l1) / n2
        a0, a1 = px * A2 - A0, py * A2 - A1
        b0, b1 = bv0 - px * bv2, bv1 - py * bv2
        lam, w = a0 * b0 + a1 * b1, a0 * a0 + a1 * a1
        z = lam / w
        zo = z * r2 + t[2]
        h0, h1 = (px - cxo) / fxo, (py - cyo) / fyo
        c0, c1, c2 = r1 - r2 * h1, r2 * h0 - r0, r0 * h1 - r1 * h0
        cn = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        dot = (r0 * h0 + r1 * h1) + r2
        par = np.arctan2(cn, dot) * RAD_TO_DEG
        flags = np.zeros(len(u), dtype=np.uint8)
        flags[~((z > 0.0) & (z < max_depth)) | ~((zo > 0.0) & (zo < max_depth))] |= CHEIRALITY
        flags[~(np.abs(d) <= max_reproj)] |= REPROJ
        flags[~(par >= min_parallax)] |= PARALLAX
        near = _near(z, 0.0) | _near(z, max_depth) | _near(zo, 0.0) | _near(zo, max_depth) | _near(np.abs(d), max_reproj)
        near |= _near(par, min_parallax)
        if certainty is not None:
            c = np.asarray(certainty, dtype=np.float64)
            flags[~(c >= min_certainty)] |= CERTAINTY
            near |= _near(c, min_certainty)
        pts = np.stack([z * x0, z * x1, z], axis=-1)
    out = {"points": pts, "depth_other": zo, "reproj": d, "parallax": par, "flags": flags, "near": near & ~degenerate}
    for k in ("points", "depth_other", "reproj", "parallax"):
        out[k] = np.where(degenerate.reshape((-1,) + (1,) * (out[k].ndim - 1)), np.nan, out[k])
    out["flags"] = np.where(degenerate, np.uint8(DEGENERATE), flags).astype(np.uint8)
    return out


def to_pixels(x, W, H):
    """the kernel's coords = 1 rule: pixel = (x + 1) * W / 2 in float64"""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([(x[..., 0] + 1.0) * float(W) / 2.0, (x[..., 1] + 1.0) * float(H) / 2.0], axis=-1)


def triangulate(matches, R, t, K_a=None, K_b=None, certainty=None, count=None, valid=True, coords=0, sizes=None, sym_w=0,
                max_depth=np.inf, max_reproj=np.inf, min_parallax=0.0, min_certainty=0.0):
    """roma_op_triangulate for ONE pair: matches [n, 4] (float32 as the device reads them, or float64), (R, t) from A to B,
    sizes = (W_a, H_a, W_b, H_b) for coords = 1.  Returns a dict: points [n, 3], depth_other, reproj, parallax [n] float64 (the
    device rounds them to float32), flags uint8 [n], stats int32 [2, 8], near bool [n]."""
    m = np.asarray(matches, dtype=np.float64).reshape(-1, 4)
    n = len(m)
    rows = n if count is None else max(0, min(int(count), n))
    if not valid:
        rows = 0
    idx = np.arange(n)
    is_b = (idx % (2 * sym_w) >= sym_w) if sym_w else np.zeros(n, dtype=bool)
    live = idx < rows
    out = {"points": np.full((n, 3), np.nan), "depth_other": np.full(n, np.nan), "reproj": np.full(n, np.nan),
           "parallax": np.full(n, np.nan), "flags": np.full(n, SKIPPED, dtype=np.uint8), "near": np.zeros(n, dtype=bool)}
    stats = np.zeros((2, 8), dtype=np.int32)
    a, b = m[:, 0:2], m[:, 2:4]
    if coords:
        a, b = to_pixels(a, sizes[0], sizes[1]), to_pixels(b, sizes[2], sizes[3])
    Ri, ti = inverse_pose(R, t)
    kw = dict(max_depth=max_depth, max_reproj=max_reproj, min_parallax=min_parallax, min_certainty=min_certainty)
    for half, sel in ((0, live & ~is_b), (1, live & is_b)):
        if not sel.any():
            continue
        cert = None if certainty is None else np.asarray(certainty).reshape(-1)[sel]
        if half == 0:
            o = triangulate_view(a[sel], b[sel], R, t, K_a, K_b, cert, **kw)
        else:
            o = triangulate_view(b[sel], a[sel], Ri, ti, K_b, K_a, cert, **kw)
        for k, v in o.items():
            out[k][sel] = v
        f = o["flags"]
        stats[half, :7] = [len(f), int((f == 0).sum())] + [int(((f & bit) != 0).sum()) for bit in (DEGENERATE, CHEIRALITY, REPROJ,
                                                                                               PARALLAX, CERTAINTY)]
    out["stats"] = stats
    return out


def depth_consistency(points, flags, R, t, K_a, K_b, sizes, H, W, rel_thresh=0.05):
    """roma_op_depth_consistency for ONE pair: points [H * 2W, 3] as the device stored them (float32) and flags [H * 2W] of a
    sym_w = W triangulation, sizes = (W_a, H_a, W_b, H_b).  Returns (consistent uint8 [H, 2W] of 0 / 1 / 2, err float64 [H, 2W],
    NaN where there is no support, near bool [H, 2W])."""
    P = np.asarray(points, dtype=np.float64).reshape(H, 2 * W, 3)
    F = np.asarray(flags).reshape(H, 2 * W)
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3)
    cons = np.full((H, 2 * W), 2, dtype=np.uint8)
    err = np.full((H, 2 * W), np.nan)
    Z = P[..., 2]
    for half in (0, 1):
        X = P[:, half * W:(half + 1) * W]
        X0, X1, X2 = X[..., 0], X[..., 1], X[..., 2]
        own = F[:, half * W:(half + 1) * W] == 0
        with np.errstate(all="ignore"):
            if half == 0:
                y0 = ((R[0, 0] * X0 + R[0, 1] * X1) + R[0, 2] * X2) + t[0]
                y1 = ((R[1, 0] * X0 + R[1, 1] * X1) + R[1, 2] * X2) + t[1]
                y2 = ((R[2, 0] * X0 + R[2, 1] * X1) + R[2, 2] * X2) + t[2]
                fx, fy, cx, cy = _cam(K_b)
                wo, ho, off = float(sizes[2]), float(sizes[3]), W
            else:
                d0, d1, d2 = X0 - t[0], X1 - t[1], X2 - t[2]
                y0 = (R[0, 0] * d0 + R[1, 0] * d1) + R[2, 0] * d2
                y1 = (R[0, 1] * d0 + R[1, 1] * d1) + R[2, 1] * d2
                y2 = (R[0, 2] * d0 + R[1, 2] * d1) + R[2, 2] * d2
                fx, fy, cx, cy = _cam(K_a)
                wo, ho, off = float(sizes[0]), float(sizes[1]), 0
            px, py = fx * (y0 / y2) + cx, fy * (y1 / y2) + cy
            gx, gy = px / wo * float(W) - 0.5, py / ho * float(H) - 0.5
            fx0, fy0 = np.floor(gx), np.floor(gy)
            inside = own & (fx0 >= 0.0) & (fx0 + 1.0 <= float(W) - 1.0) & (fy0 >= 0.0) & (fy0 + 1.0 <= float(H) - 1.0)
            xi = np.where(inside, fx0, 0).astype(np.int64) + off
            yi = np.where(inside, fy0, 0).astype(np.int64)
            xj, yj = np.minimum(xi + 1, 2 * W - 1), np.minimum(yi + 1, H - 1)  # clipped only where `inside` is false
            sup = inside & (F[yi, xi] == 0) & (F[yi, xj] == 0) & (F[yj, xi] == 0) & (F[yj, xj] == 0)
            d00, d01, d10, d11 = Z[yi, xi], Z[yi, xj], Z[yj, xi], Z[yj, xj]
            ax, ay = gx - fx0, gy - fy0
            v = (d00 * (1.0 - ax) + d01 * ax) * (1.0 - ay) + (d10 * (1.0 - ax) + d11 * ax) * ay
            e = np.abs(v - y2) / v
            c = np.where(e < rel_thresh, 1, 0)
        cons[:, half * W:(half + 1) * W] = np.where(sup, c, 2)
        err[:, half * W:(half + 1) * W] = np.where(sup, e, np.nan)
    near = _near(err, rel_thresh) & (cons != 2)
    return cons, err, near
