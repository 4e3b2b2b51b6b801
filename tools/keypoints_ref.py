"""numpy float32 restatement of roma_op_match_keypoints (include/roma_hip.h, csrc/keypoints_batched.hip): the oracle of
tests/test_gpu_keypoints_batched.py.  Brute force: the full na x nb matrix of squared distances per pair, its row and column
minima, and numpy.nonzero of the reference's mask (romatch/models/matcher.py:756-762).

Every step is float32.  The one place where the device rounds once and numpy twice is d2 = fmaf(dy, dy, dx * dx): here dy * dy is
exact in float64, the sum is rounded to float64 and then to float32.  Which pairs are mutual minima depends on comparisons of
distances only, so the two agree wherever a row's or column's minimum is not within rounding of the next distance: `min_gap`
measures that, and tests/keypoints_cases.py asserts it for every case a device test uses."""
import numpy as np

f32 = np.float32


def sample_warp_at(warp, cert, x):
    """p [n, 2], c [n]: bilinear, zeros padding, align_corners=False of warp[..., 2:4] [H, W, 2] and cert [H, W] at x [n, 2]
    normalised (x, y) - sample_warp_at_kernel's expression (without its fused multiply-adds)"""
    warp, cert, x = np.asarray(warp, f32), np.asarray(cert, f32), np.asarray(x, f32).reshape(-1, 2)
    H, W = cert.shape
    with np.errstate(invalid="ignore", over="ignore"):
        ix = ((x[:, 0] + f32(1)) * f32(W) - f32(1)) * f32(0.5)
        iy = ((x[:, 1] + f32(1)) * f32(H) - f32(1)) * f32(0.5)
        # fminf(fmaxf(v, -1e6), 1e6): a NaN becomes -1e6
        ix = np.fmin(np.fmax(ix, f32(-1.0e6)), f32(1.0e6))
        iy = np.fmin(np.fmax(iy, f32(-1.0e6)), f32(1.0e6))
    fx0, fy0 = np.floor(ix), np.floor(iy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    tx, ty = ix - fx0, iy - fy0
    wgt = [(f32(1) - tx) * (f32(1) - ty), tx * (f32(1) - ty), (f32(1) - tx) * ty, tx * ty]
    bx, by, c = (np.zeros(len(x), f32) for _ in range(3))
    for t in range(4):
        yy, xx = y0 + (t >> 1), x0 + (t & 1)
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        ys, xs = np.where(ok, yy, 0), np.where(ok, xx, 0)
        with np.errstate(invalid="ignore"):
            bx = np.where(ok, bx + wgt[t] * warp[ys, xs, 2], bx)
            by = np.where(ok, by + wgt[t] * warp[ys, xs, 3], by)
            c = np.where(ok, c + wgt[t] * cert[ys, xs], c)
    return np.stack([bx, by], axis=-1).astype(f32), c.astype(f32)


def squared_distances(p, q):
    """d2 [len(p), len(q)] float32 = fmaf(dy, dy, dx * dx) with (dx, dy) = p_i - q_j"""
    p, q = np.asarray(p, f32).reshape(-1, 2), np.asarray(q, f32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = p[:, None, 0] - q[None, :, 0]
        dy = p[:, None, 1] - q[None, :, 1]
        return (dy.astype(np.float64) * dy.astype(np.float64) + (dx * dx).astype(np.float64)).astype(f32)


def _nanmin(d2, axis):
    """the minimum that ignores NaN (a NaN distance is never a minimum); +inf where there is nothing else"""
    return np.min(np.where(np.isnan(d2), f32(np.inf), d2), axis=axis, initial=f32(np.inf))


def match_pair(x_a, x_b, warp, cert, max_dist=0.005, cert_th=0):
    """one pair: (inds [n, 2] int64 row-major, p [na, 2], c [na], d2 [na, nb])"""
    x_a, x_b = np.asarray(x_a, f32).reshape(-1, 2), np.asarray(x_b, f32).reshape(-1, 2)
    p, c = sample_warp_at(warp, cert, x_a)
    d2 = squared_distances(p, x_b)
    if d2.size == 0:
        return np.zeros((0, 2), np.int64), p, c, d2
    max_d2 = f32(max_dist) * f32(max_dist)
    with np.errstate(invalid="ignore"):
        mask = (d2 == _nanmin(d2, 1)[:, None]) & (d2 == _nanmin(d2, 0)[None, :]) & (c > f32(cert_th))[:, None] & (d2 < max_d2)
    i, j = np.nonzero(mask)  # row-major
    return np.stack([i, j], axis=-1).astype(np.int64), p, c, d2


def to_pixels(x, H, W):
    """to_pixel_coordinates: (W * 0.5f) * (x + 1.0f), (H * 0.5f) * (y + 1.0f) in float32"""
    x = np.asarray(x, f32)
    return np.stack([(f32(W) * f32(0.5)) * (x[..., 0] + f32(1)), (f32(H) * f32(0.5)) * (x[..., 1] + f32(1))], axis=-1).astype(f32)


def match_keypoints(x_A, x_B, warp, cert, counts_A=None, counts_B=None, max_dist=0.005, cert_th=0, max_matches=None, sizes=None):
    """The batched call: x_A [B, NA, 2], x_B [B, NB, 2], warp [B, H, W, 4], cert [B, H, W]; sizes None, four numbers or [B, 4].
    Returns dict(kpts_A, kpts_B [B, M, 2] f32, inds [B, M, 2] int32, counts [B] int32, total [B] int64)."""
    x_A, x_B = np.asarray(x_A, f32), np.asarray(x_B, f32)
    B, NA, NB = x_A.shape[0], x_A.shape[1], x_B.shape[1]
    M = max(NA, NB, 1) if max_matches is None else int(max_matches)
    out = dict(kpts_A=np.zeros((B, M, 2), f32), kpts_B=np.zeros((B, M, 2), f32), inds=np.full((B, M, 2), -1, np.int32),
               counts=np.zeros(B, np.int32), total=np.zeros(B, np.int64))
    if sizes is not None:
        sizes = np.broadcast_to(np.asarray(sizes, f32).reshape(-1, 4), (B, 4))
    for b in range(B):
        na = NA if counts_A is None else min(max(int(counts_A[b]), 0), NA)
        nb = NB if counts_B is None else min(max(int(counts_B[b]), 0), NB)
        inds = match_pair(x_A[b, :na], x_B[b, :nb], warp[b], cert[b], max_dist, cert_th)[0]
        n = min(len(inds), M)
        ka, kb = x_A[b, inds[:n, 0]], x_B[b, inds[:n, 1]]
        if sizes is not None:
            ka, kb = to_pixels(ka, sizes[b, 0], sizes[b, 1]), to_pixels(kb, sizes[b, 2], sizes[b, 3])
        out["total"][b], out["counts"][b] = len(inds), n
        out["inds"][b, :n], out["kpts_A"][b, :n], out["kpts_B"][b, :n] = inds[:n], ka, kb
    return out


def min_gap(d2):
    """smallest relative gap, over every row and every column of d2, between the minimum and the next DISTINCT value (equal bits -
    duplicate keypoints - tie in any arithmetic and are not a gap); inf where a line has one distinct value"""
    d2 = np.asarray(d2, np.float64)
    worst = np.inf
    for m in (d2, d2.T):
        if m.size == 0:
            continue
        lo = m.min(axis=1, keepdims=True)
        nxt = np.where(m > lo, m, np.inf).min(axis=1)
        ok = np.isfinite(nxt)
        if ok.any():
            worst = min(worst, float(((nxt[ok] - lo[ok, 0]) / nxt[ok]).min()))
    return worst
