"""numpy restatement of roma_op_keypoints_from_matches (include/roma_hip.h; roma_amd.keypoints_from_matches): the oracle of
tests/test_gpu_set_keypoints.py, written from the header's nine steps.  One problem at a time.

Every float is float32 and every product or sum is rounded once, as the header says; the one fused expression,
d2 = fmaf(dy, dy, dx * dx), is evaluated exactly: dy * dy is exact in float64, the float64 sum is corrected to round-to-odd with
the error term of the addition, and a round-to-odd float64 rounds to the same float32 as the exact sum does.  So the comparisons
with radius^2 and between distances are the device's, bit for bit."""
from __future__ import annotations

import numpy as np

f32, f64, u64, i64 = np.float32, np.float64, np.uint64, np.int64
MAX_VIEWS, MAX_PAIRS, MAX_KPTS, MAX_CELL, MAX_SIZE, MAX_GRID = 8, 64, 1 << 16, 64, 65535, 1 << 22
LOW = 0xFFFFFFFF


def fma_sq(dy, dx):
    """fl32(dy * dy + fl32(dx * dx)) with one rounding of the sum"""
    dy, dx = np.asarray(dy, f32), np.asarray(dx, f32)
    a = dy.astype(f64) * dy.astype(f64)  # 48 bits: exact
    b = (dx * dx).astype(f64)
    s = a + b
    t = s - a
    e = (a - (s - t)) + (b - t)  # a + b = s + e exactly
    bits = np.ascontiguousarray(s).view(i64)
    fix = (e != 0) & ((bits & 1) == 0)  # inexact and even: the odd neighbour on the side of the exact sum (s >= 0)
    bits = np.where(fix, bits + np.where(e > 0, 1, -1), bits)
    return bits.view(f64).astype(f32)


def to_pixels(x, y, H, W):
    with np.errstate(invalid="ignore", over="ignore"):
        return (f32(W) * f32(0.5)) * (np.asarray(x, f32) + f32(1)), (f32(H) * f32(0.5)) * (np.asarray(y, f32) + f32(1))


def grid_shape(H, W, cell):
    return (int(H) + cell - 1) // cell, (int(W) + cell - 1) // cell  # Gh, Gw


def _neighbours(radius_on):
    return [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)] if radius_on else [(0, 0)]


def keypoints_from_matches(matches, certainty, pair_views, V, sizes, counts=None, cell=2, radius=None, max_kpts=16384, one_to_one=True):
    """matches [P, N, 4] float32, certainty [P, N], pair_views [P, 2], sizes [V, 2] = (H, W), counts [P] or None.  Returns a dict:
    kpts [V, K, 2] f32, score [V, K] f32, num_kpts [V], total [V], inds [P, N, 2] int32, kept [P], info (6 ints)."""
    m = np.asarray(matches, f32)
    P, N = m.shape[:2]
    c = np.asarray(certainty, f32).reshape(P, N)
    pv = np.asarray(pair_views, dtype=i64).reshape(P, 2)
    sizes = np.asarray(sizes, dtype=i64).reshape(V, 2)
    K = int(max_kpts)
    radius = f32(cell if radius is None else radius)
    assert 2 <= V <= MAX_VIEWS and P <= MAX_PAIRS and 1 <= K <= MAX_KPTS and 1 <= cell <= MAX_CELL and 0 <= radius <= cell
    assert 2 * P * N < 2 ** 32 and (sizes >= 1).all() and (sizes <= MAX_SIZE).all()
    r2 = f32(radius * radius)
    cnt = np.full(P, N) if counts is None else np.clip(np.asarray(counts, dtype=i64), 0, N)

    # 1, 2: pixels and validity; everything per endpoint is laid out by ordinal o = (p N + n) 2 + side
    X, Y, VIEW, OK = np.zeros((P, N, 2), f32), np.zeros((P, N, 2), f32), np.zeros((P, N, 2), i64), np.zeros((P, N, 2), bool)
    for p in range(P):
        for side in range(2):
            v = int(pv[p, side])
            H, W = sizes[v]
            x, y = to_pixels(m[p, :, 2 * side], m[p, :, 2 * side + 1], H, W)
            with np.errstate(invalid="ignore"):
                OK[p, :, side] = np.isfinite(x) & np.isfinite(y) & (x >= 0) & (x < f32(W)) & (y >= 0) & (y < f32(H))
            X[p, :, side], Y[p, :, side], VIEW[p, :, side] = x, y, v
    read = np.arange(N)[None, :] < cnt[:, None]
    with np.errstate(invalid="ignore"):
        row_ok = read & np.isfinite(c) & (c > 0) & OK.all(axis=2)
    rows_read, rows_invalid = int(read.sum()), int((read & ~row_ok).sum())
    X, Y, VIEW = X.reshape(-1), Y.reshape(-1), VIEW.reshape(-1)
    E_OK = np.repeat(row_ok.reshape(-1), 2)
    ordinal = np.arange(2 * P * N, dtype=u64)
    KEY = (np.repeat(c.reshape(-1), 2).view(np.uint32).astype(u64) << u64(32)) | (u64(LOW) - ordinal)
    # 3: cells
    safe_x, safe_y = np.where(E_OK, X, 0), np.where(E_OK, Y, 0)
    CX, CY = np.floor(safe_x).astype(i64) // cell, np.floor(safe_y).astype(i64) // cell

    kpts, score = np.full((V, K, 2), np.nan, f32), np.zeros((V, K), f32)
    num_kpts, total = np.zeros(V, np.int32), np.zeros(V, np.int32)
    assigned = np.full(2 * P * N, -1, i64)
    suppressed = 0
    nb = _neighbours(radius > 0)
    for v in range(V):
        Gh, Gw = grid_shape(sizes[v, 0], sizes[v, 1], cell)
        assert Gh * Gw <= MAX_GRID
        e = np.nonzero(E_OK & (VIEW == v))[0]
        # 4: the candidate of a cell is its largest key; the ordinal in the key names the endpoint
        grid = np.zeros(Gh * Gw, u64)
        np.maximum.at(grid, CY[e] * Gw + CX[e], KEY[e])
        occ = np.nonzero(grid)[0]
        key = grid[occ]
        who = (LOW - (key & u64(LOW)).astype(i64))
        px, py, cy, cx = X[who], Y[who], occ // Gw, occ % Gw
        # 5: suppression, one pass over the candidates
        gone = np.zeros(len(occ), bool)
        if radius > 0:
            for dy, dx in nb:
                if dy == 0 and dx == 0:
                    continue
                ny, nx = cy + dy, cx + dx
                inside = (ny >= 0) & (ny < Gh) & (nx >= 0) & (nx < Gw)
                other = np.where(inside, grid[np.where(inside, ny * Gw + nx, 0)], u64(0))
                bigger = other > key
                ow = np.where(bigger, LOW - (other & u64(LOW)).astype(i64), 0)
                gone |= bigger & (fma_sq(py - Y[ow], px - X[ow]) <= r2)
        suppressed += int(gone.sum())
        surv = ~gone
        total[v] = int(surv.sum())
        # 6: the cut
        if total[v] > K:
            thr = np.sort(key[surv])[-K]
            surv &= key >= thr
        # 7: numbering in ascending cell id
        cells = occ[surv]
        n = len(cells)
        num_kpts[v] = n
        kpts[v, :n, 0], kpts[v, :n, 1] = px[surv], py[surv]
        score[v, :n] = (key[surv] >> u64(32)).astype(np.uint32).view(f32)
        index = np.full(Gh * Gw, -1, i64)
        index[cells] = np.arange(n)
        # 8: assignment of every valid endpoint of the view
        best, bestd, bestkey = np.full(len(e), -1, i64), np.zeros(len(e), f32), np.zeros(len(e), u64)
        for dy, dx in nb:
            ny, nx = CY[e] + dy, CX[e] + dx
            inside = (ny >= 0) & (ny < Gh) & (nx >= 0) & (nx < Gw)
            g = np.where(inside, ny * Gw + nx, 0)
            j = np.where(inside, index[g], -1)
            has = j >= 0
            js = np.where(has, j, 0)
            if radius > 0:
                d = fma_sq(Y[e] - kpts[v, js, 1], X[e] - kpts[v, js, 0])
                has &= d <= r2
            else:
                d = np.zeros(len(e), f32)
            k = grid[g]
            take = has & ((best < 0) | (d < bestd) | ((d == bestd) & (k > bestkey)))
            best, bestd, bestkey = np.where(take, j, best), np.where(take, d, bestd), np.where(take, k, bestkey)
        assigned[e] = best

    pairs_idx = assigned.reshape(P, N, 2)
    have = row_ok & (pairs_idx >= 0).all(axis=2)
    no_kpt = int((row_ok & ~have).sum())
    # 9: one to one, a single pass per pair
    dropped = 0
    if one_to_one:
        rowkey = (c.view(np.uint32).astype(u64) << u64(32)) | (u64(LOW) - np.arange(N, dtype=u64))[None, :]
        stay = have.copy()
        for p in range(P):
            r = np.nonzero(have[p])[0]
            for side in range(2):
                top = np.zeros(K, u64)
                np.maximum.at(top, pairs_idx[p, r, side], rowkey[p, r])
                stay[p, r] &= top[pairs_idx[p, r, side]] == rowkey[p, r]
        dropped = int((have & ~stay).sum())
        have = stay
    inds = np.where(have[..., None], pairs_idx, -1).astype(np.int32)
    kept = have.sum(axis=1).astype(np.int32)
    return dict(kpts=kpts, score=score, num_kpts=num_kpts, total=total, inds=inds, kept=kept,
                info=(rows_read, rows_invalid, no_kpt, dropped, int(kept.sum()), suppressed))
