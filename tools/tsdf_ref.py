"""numpy restatement of roma_op_tsdf_integrate, roma_op_tsdf_extract_mesh and roma_op_points_bounds (csrc/tsdf.hip; the definition
is in include/roma_hip_tsdf.h) - the oracle of tests/test_gpu_tsdf.py.  float64 where the device is float64, float32 operation by
operation where it is float32, every expression written with elementwise + - * / floor sqrt in the order the kernels use, so both
sides round alike: the device is held to it bit for bit.

Both operators report, per kind of float decision, the smallest relative distance of any decision they took to its threshold
(`margins`, a dict that the caller passes and that is updated in place): the two floors of the projection ("floor_u", "floor_v"),
z > near ("near"), sdf >= -trunc ("trunc"), the clamp at 1 and the colour's sdf <= trunc ("clamp"), the bounds of the grid
("grid"), weight >= min_weight ("min_weight") and tsdf < 0 ("inside", an absolute distance: the threshold is 0).  A case whose
margins are above 1e-9 has no borderline decision: a device that differs from it is wrong."""
from __future__ import annotations

import itertools

import numpy as np

MAX_VIEWS = 8
KINDS = ("floor_u", "floor_v", "near", "trunc", "clamp", "grid", "min_weight", "inside")


def _note(margins, kind, value):
    if margins is not None:
        margins[kind] = min(margins.get(kind, np.inf), float(value))


def _rel_margin(q, thr):
    """smallest |q - thr| / |thr| over an array, |q - thr| where thr is 0 (inf for an empty one)"""
    q = np.asarray(q, dtype=np.float64)
    q = q[np.isfinite(q)]
    if q.size == 0:
        return np.inf
    return float(np.min(np.abs(q - thr)) / (abs(thr) if thr != 0 else 1.0))


def _floor_margin(g):
    """smallest distance of a grid position to an integer, relative to max(1, |g|)"""
    g = np.asarray(g, dtype=np.float64)
    g = g[np.isfinite(g)]
    if g.size == 0:
        return np.inf
    f = g - np.floor(g)
    return float(np.min(np.minimum(f, 1.0 - f) / np.maximum(1.0, np.abs(g))))


def fresh(dims, color=False):
    """(tsdf, weight, color or None) of an empty volume of dims = (nz, ny, nx)"""
    dims = tuple(int(d) for d in dims)
    return (np.ones(dims, dtype=np.float32), np.zeros(dims, dtype=np.float32), np.zeros(dims + (3,), dtype=np.float32) if color else None)


def integrate(tsdf, weight, color, depth, K, R, t, origin, voxel_size, trunc, *, depth_weight=None, images=None, view_valid=None,
              max_weight=64.0, near=0.0, margins=None):
    """One problem: depth [V, H, W] float32, K [V, 3, 3], R [V, 3, 3], t [V, 3] float64, images V uint8 arrays [h, w, 3] -> the new
    (tsdf, weight, color); the inputs are not written."""
    tsdf, weight = np.array(tsdf, dtype=np.float32), np.array(weight, dtype=np.float32)
    color = None if color is None else np.array(color, dtype=np.float32)
    depth = np.asarray(depth, dtype=np.float32)
    V, H, W = depth.shape
    nz, ny, nx = tsdf.shape
    K, R, t = (np.asarray(a, dtype=np.float64) for a in (K, R, t))
    origin, vs, trunc = np.asarray(origin, dtype=np.float64), float(voxel_size), float(trunc)
    if not vs > 0 or not trunc > 0:
        return tsdf, weight, color
    max_weight = np.float32(max_weight)
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    X0, X1, X2 = origin[0] + (i + 0.5) * vs, origin[1] + (j + 0.5) * vs, origin[2] + (k + 0.5) * vs
    with np.errstate(all="ignore"):
        for v in range(V):
            if view_valid is not None and not view_valid[v]:
                continue
            r, tv = R[v], t[v]
            fx, fy, cx, cy = K[v, 0, 0], K[v, 1, 1], K[v, 0, 2], K[v, 1, 2]
            y0 = ((r[0, 0] * X0 + r[0, 1] * X1) + r[0, 2] * X2) + tv[0]
            y1 = ((r[1, 0] * X0 + r[1, 1] * X1) + r[1, 2] * X2) + tv[1]
            z = ((r[2, 0] * X0 + r[2, 1] * X1) + r[2, 2] * X2) + tv[2]
            live = z > near
            _note(margins, "near", _rel_margin(z, near))
            u, vv = fx * (y0 / z) + cx, fy * (y1 / z) + cy
            fu, fv = np.floor(u), np.floor(vv)
            _note(margins, "floor_u", _floor_margin(u[live]))
            _note(margins, "floor_v", _floor_margin(vv[live]))
            _note(margins, "grid", min(_rel_margin(u[live], 0.0), _rel_margin(u[live], float(W)), _rel_margin(vv[live], 0.0),
                                       _rel_margin(vv[live], float(H))))
            live &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            c, rr = np.where(live, fu, 0).astype(np.int64), np.where(live, fv, 0).astype(np.int64)
            d = depth[v][rr, c]
            w = np.ones_like(d) if depth_weight is None else np.asarray(depth_weight, dtype=np.float32)[v][rr, c]
            live &= np.isfinite(d) & (d > 0) & np.isfinite(w) & (w > 0)
            sdf = d.astype(np.float64) - z
            _note(margins, "trunc", _rel_margin(sdf[live], -trunc))
            live &= ~(sdf < -trunc)
            q = sdf / trunc
            _note(margins, "clamp", _rel_margin(q[live], 1.0))
            f = np.where(q < 1.0, q, 1.0).astype(np.float32)
            den = weight + w
            new_t = (weight * tsdf + w * f) / den
            if color is not None:
                im = np.asarray(images[v])
                ix, iy = ((2 * c + 1) * im.shape[1]) // (2 * W), ((2 * rr + 1) * im.shape[0]) // (2 * H)
                px = im[iy, ix].astype(np.float32)
                new_c = (weight[..., None] * color + w[..., None] * px) / den[..., None]
                color = np.where((live & (sdf <= trunc))[..., None], new_c, color).astype(np.float32)
            tsdf = np.where(live, new_t, tsdf).astype(np.float32)
            weight = np.where(live, np.where(den < max_weight, den, max_weight), weight).astype(np.float32)
    return tsdf, weight, color


# ------------------------------------------------------------------------------------------------------------------ extraction
PERMS = list(itertools.permutations(range(3)))  # lexicographic: the order of the tetrahedra of a cell
TET_CORNER = [[0, 1 << a, (1 << a) | (1 << b), 7] for a, b, c in PERMS]
EDGE_END = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _parity(p):
    """0 for an even permutation of 0 .. len(p) - 1, 1 for an odd one"""
    p, n = list(p), 0
    for i in range(len(p)):
        while p[i] != i:
            q = p[i]
            p[i], p[q] = p[q], p[i]
            n ^= 1
    return n


TET_ODD = [_parity(p) for p in PERMS]


def tet_table():
    """(ntri [16], tri [16][6]) of a positively oriented tetrahedron by the rule of csrc/tsdf.hip: with (i, j, k, l) an even
    permutation of the corners, one corner i inside gives (ij, ik, il), one corner i outside (ij, il, ik), i < j inside and k, l
    outside the quadrilateral (ik, il, jl, jk) cut along ik - jl."""
    def edge(a, b):
        return EDGE_END.index((min(a, b), max(a, b)))
    ntri, tris = [], []
    for case in range(16):
        ins = [n for n in range(4) if case >> n & 1]
        out = [n for n in range(4) if not case >> n & 1]
        row = []
        if len(ins) in (1, 3):
            i = ins[0] if len(ins) == 1 else out[0]
            j, k, l = [n for n in range(4) if n != i]
            if _parity((i, j, k, l)):
                k, l = l, k
            row = [edge(i, j), edge(i, k), edge(i, l)] if len(ins) == 1 else [edge(i, j), edge(i, l), edge(i, k)]
        elif len(ins) == 2:
            (i, j), (k, l) = ins, out
            if _parity((i, j, k, l)):
                k, l = l, k
            quad = [edge(i, k), edge(i, l), edge(j, l), edge(j, k)]
            row = [quad[0], quad[1], quad[2], quad[0], quad[2], quad[3]]
        ntri.append(len(row) // 3)
        tris.append(row + [0] * (6 - len(row)))
    return ntri, tris


TET_NTRI, TET_TRI = tet_table()
_POP7 = np.array([bin(m).count("1") for m in range(128)], dtype=np.int64)


def _shifted(a, o, fill):
    """a[k + oz, j + oy, i + ox] for the bit set o = ox | oy << 1 | oz << 2, `fill` beyond the grid"""
    ox, oy, oz = o & 1, o >> 1 & 1, o >> 2
    out = np.full(a.shape, fill, dtype=a.dtype)
    nz, ny, nx = a.shape[:3]
    out[:nz - oz, :ny - oy, :nx - ox] = a[oz:, oy:, ox:]
    return out


def _gradient(tsdf, valid):
    """central differences of tsdf [nz, ny, nx, 3] in (x, y, z) order and whether the six neighbours are there and valid"""
    g = np.zeros(tsdf.shape + (3,), dtype=np.float64)
    ok = np.zeros(tsdf.shape, dtype=bool)
    ok[1:-1, 1:-1, 1:-1] = True
    T = tsdf.astype(np.float64)
    for a, axis in enumerate((2, 1, 0)):
        hi, lo = [slice(1, -1)] * 3, [slice(1, -1)] * 3
        hi[axis], lo[axis] = slice(2, None), slice(0, -2)
        g[1:-1, 1:-1, 1:-1, a] = T[tuple(hi)] - T[tuple(lo)]
        ok[1:-1, 1:-1, 1:-1] &= valid[tuple(hi)] & valid[tuple(lo)]
    return g, ok


def extract_mesh(tsdf, weight, color, origin, voxel_size, *, min_weight=1.0, max_vertices=None, max_faces=None, margins=None):
    """One problem -> dict(vertices, normals, colors, faces, counts, totals, stats), padded as the device pads them."""
    tsdf, weight = np.asarray(tsdf, dtype=np.float32), np.asarray(weight, dtype=np.float32)
    nz, ny, nx = tsdf.shape
    G = nz * ny * nx
    if max_vertices is None:
        max_vertices = 16 * (nx * ny + ny * nz + nx * nz)
    if max_faces is None:
        max_faces = 2 * max_vertices
    origin, vs = np.asarray(origin, dtype=np.float64), float(voxel_size)
    with np.errstate(all="ignore"):
        valid = weight >= np.float32(min_weight)
        if not vs > 0:
            valid = np.zeros_like(valid)
        inside = valid & (tsdf < 0)
        _note(margins, "min_weight", _rel_margin(weight, float(np.float32(min_weight))))
        _note(margins, "inside", _rel_margin(tsdf[valid], 0.0))
        vb = [_shifted(valid, o, False) for o in range(8)]
        ib = [_shifted(inside, o, False) for o in range(8)]
        has = np.stack([vb[0] & vb[c] & (ib[0] != ib[c]) for c in range(1, 8)], axis=-1).reshape(G, 7)
        mask = (has * (1 << np.arange(7))).sum(axis=1).astype(np.int64)
        base = np.cumsum(_POP7[mask]) - _POP7[mask]
        q, cm1 = np.nonzero(has)  # (grid point, edge class) order
        total_v = len(q)
        cls = cm1 + 1
        k, j, i = np.unravel_index(q, (nz, ny, nx))
        d = np.stack([cls & 1, cls >> 1 & 1, cls >> 2], axis=1)
        far = ((k + d[:, 2]) * ny + (j + d[:, 1])) * nx + (i + d[:, 0])
        T = tsdf.reshape(G).astype(np.float64)
        f0, f1 = T[q], T[far]
        s = f0 / (f0 - f1)
        ijk = np.stack([i, j, k], axis=1).astype(np.float64)
        verts = (origin[None, :] + ((ijk + 0.5) + s[:, None] * d) * vs).astype(np.float32)
        g, gok = _gradient(tsdf, valid)
        g, gok = g.reshape(G, 3), gok.reshape(G)
        gi = g[q] + s[:, None] * (g[far] - g[q])
        length = np.sqrt((gi[:, 0] * gi[:, 0] + gi[:, 1] * gi[:, 1]) + gi[:, 2] * gi[:, 2])
        good = gok[q] & gok[far] & (length > 0)
        normals = np.where(good[:, None], gi / length[:, None], np.nan).astype(np.float32)
        cols = None
        if color is not None:
            C = np.asarray(color, dtype=np.float32).reshape(G, 3).astype(np.float64)
            c = C[q] + s[:, None] * (C[far] - C[q])
            c = np.where(c > 0.0, c, 0.0)
            c = np.where(c < 255.0, c, 255.0)
            cols = np.floor(c + 0.5).astype(np.uint8)
        # faces in (cell, tetrahedron, triangle) order
        exists = np.zeros((G, 6, 2), dtype=bool)
        names = np.zeros((G, 6, 2, 3), dtype=np.int64)
        K_, J_, I_ = np.unravel_index(np.arange(G), (nz, ny, nx))
        for tau in range(6):
            o = TET_CORNER[tau]
            whole = (vb[o[0]] & vb[o[1]] & vb[o[2]] & vb[o[3]]).reshape(G)
            case = sum(ib[o[n]].reshape(G).astype(np.int64) << n for n in range(4))
            ntri = np.where(whole, np.asarray(TET_NTRI)[case], 0)
            vn = []
            for e in range(6):  # the vertex number of every edge of the tetrahedron, where its owner is in the grid
                oa, ob = o[EDGE_END[e][0]], o[EDGE_END[e][1]]
                c = oa ^ ob
                owner = (np.minimum(K_ + (oa >> 2), nz - 1) * ny + np.minimum(J_ + (oa >> 1 & 1), ny - 1)) * nx + np.minimum(I_ + (oa & 1), nx - 1)
                vn.append(base[owner] + _POP7[mask[owner] & ((1 << (c - 1)) - 1)])
            vn = np.stack(vn, axis=1)  # [G, 6]
            tri = np.asarray(TET_TRI)[case]  # [G, 6] edge ids
            for n in range(2):
                exists[:, tau, n] = ntri > n
                for e in range(3):
                    slot = e if not TET_ODD[tau] or e == 0 else 3 - e
                    names[:, tau, n, slot] = np.take_along_axis(vn, tri[:, 3 * n + e][:, None], axis=1)[:, 0]
        faces = names[exists]  # row-major: (cell, tetrahedron, triangle)
        total_f = len(faces)
    nv, nf = min(total_v, max_vertices), min(total_f, max_faces)
    used = np.zeros(max(nv, 1), dtype=bool)
    named = faces[faces < max_vertices]
    used[named] = True
    cut = (faces[:nf] >= max_vertices).any(axis=1) if nf else np.zeros(0, dtype=bool)
    out_f = np.full((max_faces, 3), -1, dtype=np.int32)
    out_f[:nf] = np.where(cut[:, None], -1, faces[:nf])
    out_v = np.full((max_vertices, 3), np.nan, dtype=np.float32)
    out_n = np.full((max_vertices, 3), np.nan, dtype=np.float32)
    out_v[:nv], out_n[:nv] = verts[:nv], normals[:nv]
    out_c = None
    if cols is not None:
        out_c = np.zeros((max_vertices, 3), dtype=np.uint8)
        out_c[:nv] = cols[:nv]
    stats = np.array([valid.sum(), inside.sum(), nv, nf, nv - int(used[:nv].sum()), int(cut.sum()), int(exists.any(axis=(1, 2)).sum()), 0],
                     dtype=np.int32)
    return dict(vertices=out_v, normals=out_n, colors=out_c, faces=out_f, counts=np.array([nv, nf], dtype=np.int32),
                totals=np.array([total_v, total_f], dtype=np.int32), stats=stats)


# ---------------------------------------------------------------------------------------------------------------------- bounds
def _key(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _value(key):
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32).view(np.float32)


def points_bounds(points, count=None):
    """(min, max) float64 [2, 3] of the finite rows of points [N, 3] below count, through the ordered integer image of the float
    bits (-0 sorts below +0); NaN where there is no finite row"""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(points) if count is None else min(max(int(count), 0), len(points))
    rows = points[:n]
    rows = rows[np.isfinite(rows).all(axis=1)]
    if len(rows) == 0:
        return np.full((2, 3), np.nan)
    keys = _key(rows)
    return np.stack([_value(keys.min(axis=0)), _value(keys.max(axis=0))]).astype(np.float64)


def volume_from_bounds(bounds, dims, margin=0.05):
    """(origin [3], voxel_size) of a cubic-voxel volume of dims = (nz, ny, nx) around the box bounds [2, 3]: the box grown by
    `margin` times its largest extent on every side, the voxel the largest of the three quotients, the box centred"""
    lo, hi = np.asarray(bounds, dtype=np.float64)
    n = np.array([dims[2], dims[1], dims[0]], dtype=np.float64)
    ext = hi - lo
    pad = margin * ext.max()
    vs = ((ext + 2.0 * pad) / n).max()
    return (lo + hi) * 0.5 - 0.5 * n * vs, vs
