"""numpy float64 restatement of roma_op_fuse_depth_maps and roma_op_relative_poses (csrc/depth_fusion.hip; the definition is in
include/roma_hip.h) - the oracle of tests/test_gpu_depth_fusion.py.  Every expression is written with elementwise + - * / floor in
the order the kernels use (no matrix product, whose summation order numpy does not fix), so both sides round alike: the device
is held to it bit for bit.

Besides the outputs, `fuse` reports `margin`: the smallest relative distance of any decision it took to the threshold it was
taken against - the support test |z_l - z_k| <= rel min(z_l, z_k), the seen / violated tests on e, and the floor of a grid
position (the bilinear lookup's floor(g) and the nearest pixel's floor(g + 0.5)).  A case whose margin is above 1e-9 has no
borderline decision: a device that differs from it is wrong."""
from __future__ import annotations

import numpy as np

MAX_VIEWS, MAX_PAIRS, MAX_SLOTS = 8, 64, 14


def relative_poses(R, t, pair_views):
    """R [V, 3, 3], t [V, 3] with x_cam = R X + t -> (R_ij [P, 3, 3], t_ij [P, 3]): R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i"""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    Ro, to = np.zeros((len(pair_views), 3, 3)), np.zeros((len(pair_views), 3))
    for p, (i, j) in enumerate(pair_views):
        for a in range(3):
            for c in range(3):
                Ro[p, a, c] = (R[j, a, 0] * R[i, c, 0] + R[j, a, 1] * R[i, c, 1]) + R[j, a, 2] * R[i, c, 2]
            to[p, a] = t[j, a] - ((Ro[p, a, 0] * t[i, 0] + Ro[p, a, 1] * t[i, 1]) + Ro[p, a, 2] * t[i, 2])
    return Ro, to


def slots_of(pair_views, V, symmetric):
    """for every view the (pair, half) whose half of the grid lies on it, in ascending pair"""
    out = [[] for _ in range(V)]
    for p, (i, j) in enumerate(pair_views):
        out[int(i)].append((p, 0))
        if symmetric:
            out[int(j)].append((p, 1))
    return out


def _rel_margin(q, thr):
    """smallest |q - thr| / thr over an array (inf for an empty one or a zero threshold)"""
    q = np.asarray(q, dtype=np.float64)
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), q.shape)
    ok = np.isfinite(q) & (thr > 0)
    return float(np.min(np.abs(q[ok] - thr[ok]) / thr[ok])) if ok.any() else np.inf


def _floor_margin(g):
    """smallest distance of a grid position to an integer, relative to max(1, |g|)"""
    g = np.asarray(g, dtype=np.float64)
    g = g[np.isfinite(g)]
    if g.size == 0:
        return np.inf
    f = g - np.floor(g)
    return float(np.min(np.minimum(f, 1.0 - f) / np.maximum(1.0, np.abs(g))))


def _world(cam, R, t, H, W, z):
    """X_w = R^T (z ((u - cx) / fx, (v - cy) / fy, 1) - t) of every cell centre: three [H, W] arrays"""
    fx, fy, cx, cy = cam[0, 0], cam[1, 1], cam[0, 2], cam[1, 2]
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x0, x1 = ((c + 0.5) - cx) / fx, ((r + 0.5) - cy) / fy
    d0, d1, d2 = z * x0 - t[0], z * x1 - t[1], z - t[2]
    return [(R[0, i] * d0 + R[1, i] * d1) + R[2, i] * d2 for i in range(3)]


def _project(cam, R, t, X):
    """(depth in the view, gx, gy) of world points: the grid position with the centre of cell 0 at 0"""
    fx, fy, cx, cy = cam[0, 0], cam[1, 1], cam[0, 2], cam[1, 2]
    y = [((R[i, 0] * X[0] + R[i, 1] * X[1]) + R[i, 2] * X[2]) + t[i] for i in range(3)]
    return y[2], (fx * (y[0] / y[2]) + cx) - 0.5, (fy * (y[1] / y[2]) + cy) - 0.5


def fuse(points, flags, certainty, pair_views, cameras, R, t, symmetric=True, rel_thresh=0.01, min_support=2, min_consistent=1,
         max_violations=0, dedupe=True, max_points=None, view_valid=None, valid=True, images=None):
    """roma_op_fuse_depth_maps for ONE problem.  points [P, H, Wd, 3] (or the depths [P, H, Wd]) as the device reads them
    (float32), flags uint8 [P, H, Wd], certainty [P, H, Wd] or None, pair_views P pairs (i, j), cameras [V, 3, 3] in grid units,
    R [V, 3, 3], t [V, 3]; images: None or V uint8 arrays [H_img, W_img, 3].  Returns a dict of the operator's outputs (depth,
    weight float32; support, seen, violated, state uint8 [V, H, W]; points float32 [max_points, 3], colors uint8 [max_points, 3]
    or None, cloud_weight float32, source int32 [max_points, 2], count, total, stats) and `margin`."""
    z_all = np.asarray(points)
    z_all = (z_all[..., 2] if z_all.ndim == 4 else z_all).astype(np.float32)
    flags = np.asarray(flags)
    P, H, Wd = z_all.shape
    W = Wd // 2 if symmetric else Wd
    cameras, R, t = (np.asarray(x, dtype=np.float64) for x in (cameras, R, t))
    V = len(cameras)
    rel = float(rel_thresh)
    vv = np.ones(V, dtype=bool) if view_valid is None else np.asarray(view_valid).astype(bool)
    on = vv & bool(valid)
    cert = None if certainty is None else np.asarray(certainty).astype(np.float32)
    margin = np.inf
    n = H * W
    depth = np.full((V, H, W), np.nan, dtype=np.float32)
    weight = np.zeros((V, H, W), dtype=np.float32)
    support = np.zeros((V, H, W), dtype=np.uint8)
    stats = np.zeros(8, dtype=np.int64)
    # 1 - 3: hypotheses, support, selection
    with np.errstate(all="ignore"):
        for v, slots in enumerate(slots_of(pair_views, V, symmetric)):
            if not on[v]:
                continue
            Z, Wt, U = [], [], []
            for p, half in slots:
                other = int(pair_views[p][1 - half])
                sl = np.s_[p, :, half * W:(half + 1) * W]
                zf = z_all[sl]
                wf = np.ones((H, W), dtype=np.float32) if cert is None else cert[sl]
                ok = (flags[sl] == 0) & np.isfinite(zf) & (zf > 0) & np.isfinite(wf) & (wf > 0) & bool(vv[other])
                U.append(ok)
                Z.append(np.where(ok, zf, 0).astype(np.float64))
                Wt.append(np.where(ok, wf, 0).astype(np.float64))
            if not slots:
                continue
            WZ = [w * z for w, z in zip(Wt, Z)]
            best_n = np.zeros((H, W), dtype=np.int64)
            best_s, best_num = np.zeros((H, W)), np.zeros((H, W))
            for k in range(len(slots)):
                nk = np.zeros((H, W), dtype=np.int64)
                sk, numk = np.zeros((H, W)), np.zeros((H, W))
                for l in range(len(slots)):
                    dz, thr = np.abs(Z[l] - Z[k]), rel * np.minimum(Z[l], Z[k])
                    sup = U[l] & (dz <= thr)
                    nk = nk + sup
                    sk = sk + np.where(sup, Wt[l], 0.0)
                    numk = numk + np.where(sup, WZ[l], 0.0)
                    if l != k:
                        both = U[l] & U[k]
                        margin = min(margin, _rel_margin(dz[both], thr[both]))
                better = U[k] & ((nk > best_n) | ((nk == best_n) & (sk > best_s)))
                best_n, best_s, best_num = np.where(better, nk, best_n), np.where(better, sk, best_s), np.where(better, numk, best_num)
            fused = best_n >= int(min_support)
            depth[v] = np.where(fused, best_num / best_s, np.nan).astype(np.float32)
            weight[v] = np.where(fused, best_s, 0.0).astype(np.float32)
            support[v] = best_n.astype(np.uint8)
            stats[0] += int(np.any(U, axis=0).sum())
            stats[1] += int(fused.sum())
    # 4: the cross-view check on the fused maps
    seen = np.zeros((V, H, W), dtype=np.uint8)
    violated = np.zeros((V, H, W), dtype=np.uint8)
    keep = np.zeros((V, H, W), dtype=bool)
    Xw = [None] * V
    with np.errstate(all="ignore"):
        for v in range(V):
            fusedv = ~np.isnan(depth[v])
            Xw[v] = _world(cameras[v], R[v], t[v], H, W, depth[v].astype(np.float64))
            for u in range(V):
                if u == v or not on[u]:
                    continue
                pz, gx, gy = _project(cameras[u], R[u], t[u], Xw[v])
                fx0, fy0 = np.floor(gx), np.floor(gy)
                front = fusedv & (pz > 0.0)
                inside = front & (fx0 >= 0.0) & (fx0 + 1.0 <= float(W) - 1.0) & (fy0 >= 0.0) & (fy0 + 1.0 <= float(H) - 1.0)
                margin = min(margin, _floor_margin(gx[front]), _floor_margin(gy[front]))
                xi, yi = np.where(inside, fx0, 0).astype(np.int64), np.where(inside, fy0, 0).astype(np.int64)
                xj, yj = np.minimum(xi + 1, W - 1), np.minimum(yi + 1, H - 1)  # clipped only where `inside` is false
                D = depth[u]
                f00, f01, f10, f11 = D[yi, xi], D[yi, xj], D[yj, xi], D[yj, xj]
                sup = inside & ~(np.isnan(f00) | np.isnan(f01) | np.isnan(f10) | np.isnan(f11))
                d00, d01, d10, d11 = (f.astype(np.float64) for f in (f00, f01, f10, f11))
                ax, ay = gx - fx0, gy - fy0
                d = (d00 * (1.0 - ax) + d01 * ax) * (1.0 - ay) + (d10 * (1.0 - ax) + d11 * ax) * ay
                e = (pz - d) / d
                seen[v] |= (np.where(sup & (np.abs(e) <= rel), 1, 0) << u).astype(np.uint8)
                violated[v] |= (np.where(sup & (e < -rel), 1, 0) << u).astype(np.uint8)
                margin = min(margin, _rel_margin(np.abs(e[sup]), rel))
            pop_s = sum((seen[v] >> u) & 1 for u in range(V))
            pop_v = sum((violated[v] >> u) & 1 for u in range(V))
            keep[v] = fusedv & (pop_s >= int(min_consistent)) & (pop_v <= int(max_violations))
        stats[2] = int(keep.sum())
        stats[5] = int((violated != 0).sum())
        # 5: duplicates, from `keep` alone
        dup = np.zeros((V, H, W), dtype=bool)
        if dedupe:
            for v in range(V):
                for u in range(v):
                    cand = keep[v] & (((seen[v] >> u) & 1) != 0)
                    if not cand.any():
                        continue
                    _, gx, gy = _project(cameras[u], R[u], t[u], Xw[v])
                    margin = min(margin, _floor_margin((gx + 0.5)[cand]), _floor_margin((gy + 0.5)[cand]))
                    nx, ny = np.floor(gx + 0.5), np.floor(gy + 0.5)
                    inside = cand & (nx >= 0.0) & (nx <= float(W) - 1.0) & (ny >= 0.0) & (ny <= float(H) - 1.0)
                    xi, yi = np.where(inside, nx, 0).astype(np.int64), np.where(inside, ny, 0).astype(np.int64)
                    dup[v] |= inside & keep[u][yi, xi]
        stats[3] = int(dup.sum())
    state = (keep.astype(np.uint8) | (dup.astype(np.uint8) << 1)).astype(np.uint8)
    # 6: emission in (view, row-major pixel) order
    emit = (keep & ~dup).reshape(V, n)
    vs, qs = np.nonzero(emit)
    total = len(vs)
    K = V * n if max_points is None else int(max_points)  # the default of roma_amd.fuse_depth_maps
    count = min(total, K)
    stats[4] = count
    out_points = np.full((K, 3), np.nan, dtype=np.float32)
    out_weight = np.zeros(K, dtype=np.float32)
    out_source = np.full((K, 2), -1, dtype=np.int32)
    out_colors = None if images is None else np.zeros((K, 3), dtype=np.uint8)
    vs, qs = vs[:count], qs[:count]
    for i in range(3):
        out_points[:count, i] = np.stack([x.reshape(n) for x in (X[i] for X in Xw)])[vs, qs].astype(np.float32)
    out_weight[:count] = weight.reshape(V, n)[vs, qs]
    out_source[:count, 0], out_source[:count, 1] = vs, qs
    if images is not None:
        for k, (v, q) in enumerate(zip(vs, qs)):
            im = np.asarray(images[v])
            r, c = divmod(int(q), W)
            out_colors[k] = im[((2 * r + 1) * im.shape[0]) // (2 * H), ((2 * c + 1) * im.shape[1]) // (2 * W)]
    return {"depth": depth, "weight": weight, "support": support, "seen": seen, "violated": violated, "state": state,
            "points": out_points, "colors": out_colors, "cloud_weight": out_weight, "source": out_source, "count": count,
            "total": total, "stats": tuple(int(s) for s in stats), "margin": float(margin)}
