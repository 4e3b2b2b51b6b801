"""numpy float64 restatement of roma_op_render_points (csrc/point_render.hip; the definition is in include/roma_hip.h) - the oracle
of tests/test_gpu_point_render.py.  Every expression is written with elementwise + - * / floor in the order the kernels use (no
matrix product, whose summation order numpy does not fix), so both sides round alike: the device is held to it bit for bit.  The
z-buffer is `np.minimum.at` on uint64 keys, the windows of the filter and the fill are shifted views of a padded frame.

Besides the outputs, `render` reports `margins`: for every float decision it takes, the smallest relative distance to the
threshold it was taken against -
  cell      u and v to the nearest integer (the floor that picks the cell), relative to max(1, |u|)
  near, far X'_z to near and to far
  frustum   floor(u) against -radius and W + radius (and v against H): u to those two bounds, relative to max(1, |bound|)
  occlusion z against z_q (1 + occlusion_rel), over every pair of hit pixels the filter compares
and `margin`, the smallest of them.  A case whose margin is above 1e-9 has no borderline decision: a device that differs from it is
wrong."""
from __future__ import annotations

import numpy as np

MAX_RADIUS = 4
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
HIT, REMOVED, FILLED = 1, 2, 4  # bits of `mask`


def _rel_margin(q, thr, scale=None):
    """smallest |q - thr| / scale over an array (scale: thr unless given); inf for an empty one"""
    q = np.asarray(q, dtype=np.float64)
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), q.shape)
    scale = np.abs(thr) if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), q.shape)
    ok = np.isfinite(q) & np.isfinite(thr) & (scale > 0)
    return float(np.min(np.abs(q[ok] - thr[ok]) / scale[ok])) if ok.any() else np.inf


def _floor_margin(g):
    """smallest distance of a position to an integer, relative to max(1, |g|)"""
    g = np.asarray(g, dtype=np.float64)
    g = g[np.isfinite(g)]
    if g.size == 0:
        return np.inf
    f = g - np.floor(g)
    return float(np.min(np.minimum(f, 1.0 - f) / np.maximum(1.0, np.abs(g))))


def key_depth(key):
    """the float32 depth in the upper half of uint64 keys"""
    return (np.asarray(key, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


def _windows(a, rad, pad):
    """the (2 rad + 1)^2 shifted views of frame a [H, W], padded with `pad`: what a clipped window sees"""
    H, W = a.shape
    p = np.full((H + 2 * rad, W + 2 * rad), pad, dtype=a.dtype)
    p[rad:rad + H, rad:rad + W] = a
    for dr in range(2 * rad + 1):
        for dc in range(2 * rad + 1):
            yield p[dr:dr + H, dc:dc + W]


def splat(points, cam, R, t, H, W, count, radius, near, far, margins=None):
    """step 1 for one camera: (key uint64 [H, W], usable rows with (r0, c0) inside the image)"""
    pts = np.asarray(points, dtype=np.float32)
    N = len(pts)
    n = np.arange(N, dtype=np.int64)
    fx, fy, cx, cy = cam[0, 0], cam[1, 1], cam[0, 2], cam[1, 2]
    rad = float(radius)
    with np.errstate(all="ignore"):
        ok = (n < count) & np.isfinite(pts).all(axis=1)
        X = pts.astype(np.float64)
        X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
        y = [((R[i, 0] * X0 + R[i, 1] * X1) + R[i, 2] * X2) + t[i] for i in range(3)]
        ranged = ok & (y[2] >= near) & (y[2] <= far)
        zf = y[2].astype(np.float32)
        u, v = fx * (y[0] / y[2]) + cx, fy * (y[1] / y[2]) + cy
        proj = ranged & np.isfinite(zf) & (zf > 0) & np.isfinite(u) & np.isfinite(v)
        fu, fv = np.floor(u), np.floor(v)
        usable = proj & (fu >= -rad) & (fu < float(W) + rad) & (fv >= -rad) & (fv < float(H) + rad)
    if margins is not None:
        m = margins
        m["near"] = min(m["near"], _rel_margin(y[2][ok], near))
        m["far"] = min(m["far"], _rel_margin(y[2][ok], far))
        m["cell"] = min(m["cell"], _floor_margin(u[proj]), _floor_margin(v[proj]))
        for g, size in ((u[proj], W), (v[proj], H)):
            for bound in (-rad, float(size) + rad):
                m["frustum"] = min(m["frustum"], _rel_margin(g, bound, max(1.0, abs(bound))))
    rows = n[usable]
    c0, r0 = fu[usable].astype(np.int64), fv[usable].astype(np.int64)
    keys = (zf[usable].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    key = np.full(H * W, EMPTY, dtype=np.uint64)
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            r, c = r0 + dr, c0 + dc
            on = (r >= 0) & (r < H) & (c >= 0) & (c < W)
            np.minimum.at(key, (r * W + c)[on], keys[on])
    inside = int(((r0 >= 0) & (r0 < H) & (c0 >= 0) & (c0 < W)).sum())
    return key.reshape(H, W), inside


def occlusion_filter(key, radius, rel, count, margins=None):
    """step 2: removed [H, W] bool from the raw keys"""
    hit = key != EMPTY
    removed = np.zeros(key.shape, dtype=bool)
    if radius <= 0:
        return removed
    z = key_depth(key).astype(np.float64)
    factor = 1.0 + float(rel)
    nearer = np.zeros(key.shape, dtype=np.int64)
    for kq in _windows(key, radius, EMPTY):
        hq = kq != EMPTY
        thr = key_depth(kq).astype(np.float64) * factor
        both = hit & hq
        nearer += both & (z > thr)
        if margins is not None:
            margins["occlusion"] = min(margins["occlusion"], _rel_margin(z[both], thr[both]))
    return hit & (nearer >= int(count))


def fill(key, removed, radius, fill_min):
    """step 3: (final key, filled) from step 2's decisions"""
    alive = (key != EMPTY) & ~removed
    final = np.where(alive, key, EMPTY)
    filled = np.zeros(key.shape, dtype=bool)
    if radius <= 0:
        return final, filled
    cnt = np.zeros(key.shape, dtype=np.int64)
    best = np.full(key.shape, EMPTY, dtype=np.uint64)
    for kq in _windows(final, radius, EMPTY):  # a pixel that did not survive shows as EMPTY: no count, no key
        cnt += kq != EMPTY
        best = np.minimum(best, kq)
    filled = ~alive & (cnt >= int(fill_min))
    return np.where(filled, best, final), filled


def render(points, cameras, R, t, H, W, colors=None, count=None, valid=True, radius=1, near=1e-6, far=np.inf, occlusion_radius=2,
           occlusion_rel=0.05, occlusion_count=3, fill_radius=1, fill_min=3, background=(0, 0, 0)):
    """roma_op_render_points for ONE problem.  points [N, 3] as the device reads them (float32), cameras [C, 3, 3] in output pixels,
    R [C, 3, 3], t [C, 3], colors uint8 [N, 3] or None, count: rows at and beyond it are ignored (None: all N).  Returns a dict:
    depth float32 [C, H, W], index int32, color uint8 [C, H, W, 3] or None, mask uint8, stats int [C, 4], key uint64 [C, H, W] (the raw
    buffer of step 1), margins and margin."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    cameras, R, t = (np.asarray(x, dtype=np.float64) for x in (cameras, R, t))
    C, N = len(cameras), len(pts)
    cnt = N if count is None else min(max(int(count), 0), N)
    if not valid:
        cnt = 0
    margins = {k: np.inf for k in ("cell", "near", "far", "frustum", "occlusion")}
    depth = np.full((C, H, W), np.nan, dtype=np.float32)
    index = np.full((C, H, W), -1, dtype=np.int32)
    mask = np.zeros((C, H, W), dtype=np.uint8)
    color = None if colors is None else np.empty((C, H, W, 3), dtype=np.uint8)
    raw = np.empty((C, H, W), dtype=np.uint64)
    stats = np.zeros((C, 4), dtype=np.int64)
    for k in range(C):
        key, inside = splat(pts, cameras[k], R[k], t[k], H, W, cnt, int(radius), float(near), float(far), margins)
        raw[k] = key
        removed = occlusion_filter(key, int(occlusion_radius), occlusion_rel, occlusion_count, margins)
        final, filled = fill(key, removed, int(fill_radius), fill_min)
        hit, have = key != EMPTY, final != EMPTY
        depth[k] = np.where(have, key_depth(final), np.float32(np.nan))
        row = (final & np.uint64(0xFFFFFFFF)).astype(np.int64)
        index[k] = np.where(have, row, -1)
        mask[k] = hit * HIT + removed * REMOVED + filled * FILLED
        if color is not None and N == 0:
            color[k] = np.asarray(background, dtype=np.uint8)
        elif color is not None:
            color[k] = np.where(have[..., None], np.asarray(colors, dtype=np.uint8)[np.where(have, row, 0)],
                                np.asarray(background, dtype=np.uint8))
        stats[k] = inside, hit.sum(), removed.sum(), filled.sum()
    return {"depth": depth, "index": index, "color": color, "mask": mask, "stats": stats.astype(np.int32), "key": raw,
            "margins": margins, "margin": float(min(margins.values()))}
