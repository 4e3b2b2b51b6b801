"""What the TSDF tests share (test_cpu_tsdf.py, test_gpu_tsdf.py): a hand-made 4 x 3 x 3 volume with one 4 x 4 view of one crossing
plane, whose volume and mesh are written out; analytic signed distance fields (a sphere and a torus in a 20^3 grid) that go
straight into the extraction; and integration cases on the two-plane scene of depth_fusion_cases (a tilted background plane
behind a fronto-parallel rectangle, cameras around them).  An integration case is a dict depth [V, H, W] f32, depth_weight or
None, K [V, 3, 3] in grid units, R, t, images or None, dims, origin, voxel_size, trunc, max_weight, near, view_valid."""
import functools
import os
import sys

import numpy as np

from conftest import ROOT
from depth_fusion_cases import BG_D, BG_N, FG_X, FG_Y, FG_Z, cameras_around, look_at, plane_distance, true_depth  # noqa: F401

sys.path.insert(0, os.path.join(ROOT, "tools"))
import tsdf_ref as tr  # noqa: E402

f32 = np.float32
EDGE = 1e-9  # no float decision of a case the GPU file compares may lie within this (relative) of its threshold


# ------------------------------------------------------------------------------------------------------------- the hand-made case
# Voxel centres x, y in {-1, 0, 1}, z in {1, 2, 3, 4}; one camera at the origin looking along z, f = 1.4, principal point
# (2.25, 1.75) in a 4 x 4 grid; every cell sees the plane z = 2.5 except cell (0, 0), which has no depth - the only voxel that
# projects there is (x, y, z) = (-1, -1, 1).  trunc = 2: sdf = 2.5 - z = 1.5, 0.5, -0.5, -1.5 in the four layers.
HAND_DIMS = (4, 3, 3)
HAND_ORIGIN, HAND_VOXEL, HAND_TRUNC = (-1.5, -1.5, 0.5), 1.0, 2.0
HAND_TSDF_LAYERS = (0.75, 0.25, -0.25, -0.75)
# The surface lies halfway between layers 1 and 2.  A grid point (i, j, 1) owns the crossing edges of class 4 (straight up), 5
# (up and +x), 6 (up and +y) and 7 (the body diagonal) where the far end is in the grid: 9 + 6 + 6 + 4 = 25 vertices, the 5 x 5
# half-integer lattice of [-1, 1]^2 at z = 2.5.  Each of the 4 cells has 6 tetrahedra; the two whose first axis is z have three
# corners inside (1 triangle), the two whose second axis is z have two (2 triangles), the two whose last axis is z have one (1
# triangle): 8 triangles a cell, 32 in all - a disc: 25 - 56 + 32 = 1.  Only grid points (1, 1, 1) and (1, 1, 2) have all six
# neighbours, so only the vertex between them carries a normal: (0, 0, -1), towards the camera.
HAND_VERTICES_OF_FIRST_POINT = [(-1.0, -1.0, 2.5), (-0.5, -1.0, 2.5), (-1.0, -0.5, 2.5), (-0.5, -0.5, 2.5)]  # classes 4, 5, 6, 7
HAND_COUNTS = (25, 32)
HAND_STATS = (35, 18, 25, 32, 0, 0, 4, 0)  # 36 voxels less the unseen one; the two far layers are inside


def hand_made():
    K = np.array([[[1.4, 0.0, 2.25], [0.0, 1.4, 1.75], [0.0, 0.0, 1.0]]])
    depth = np.full((1, 4, 4), 2.5, dtype=f32)
    depth[0, 0, 0] = np.nan
    return dict(depth=depth, depth_weight=None, K=K, R=np.eye(3)[None], t=np.zeros((1, 3)), images=None, dims=HAND_DIMS,
                origin=np.array(HAND_ORIGIN), voxel_size=HAND_VOXEL, trunc=HAND_TRUNC, max_weight=64.0, near=1e-6, view_valid=None)


def check_hand_made(tsdf, weight, mesh):
    """tsdf, weight [4, 3, 3] and the mesh outputs as numpy arrays (the operator's or the restatement's), min_weight = 0.5"""
    want_t = np.broadcast_to(np.asarray(HAND_TSDF_LAYERS, dtype=f32)[:, None, None], HAND_DIMS).copy()
    want_w = np.ones(HAND_DIMS, dtype=f32)
    want_t[0, 0, 0], want_w[0, 0, 0] = 1.0, 0.0
    assert np.array_equal(tsdf, want_t) and np.array_equal(weight, want_w)
    nv, nf = HAND_COUNTS
    assert tuple(mesh["counts"]) == HAND_COUNTS == tuple(mesh["totals"]) and tuple(mesh["stats"]) == HAND_STATS
    v, n, f = mesh["vertices"], mesh["normals"], mesh["faces"]
    assert [tuple(r) for r in v[:4]] == HAND_VERTICES_OF_FIRST_POINT
    lattice = sorted((x / 2.0, y / 2.0, 2.5) for x in range(-2, 3) for y in range(-2, 3))
    assert sorted(tuple(r) for r in v[:nv]) == lattice and np.isnan(v[nv:]).all() and (f[nf:] == -1).all()
    finite = np.isfinite(n[:nv]).all(axis=1)
    assert finite.sum() == 1 and tuple(v[:nv][finite][0]) == (0.0, 0.0, 2.5) and tuple(n[:nv][finite][0]) == (0.0, 0.0, -1.0)
    tri = v[f[:nf]].astype(np.float64)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (normal[:, :2] == 0).all() and (normal[:, 2] < 0).all()  # every triangle faces the camera, the positive side
    assert abs(0.5 * np.abs(normal[:, 2]).sum() - 4.0) < 1e-12      # and together they tile [-1, 1]^2
    check_topology(f[:nf], nv, euler=1, closed=False)


# ------------------------------------------------------------------------------------------------------------- analytic fields
FIELD_N, FIELD_TRUNC = 20, 4.0
SPHERE_C, SPHERE_R = (10.137, 9.927, 10.467), 6.2
TORUS_C, TORUS_R, TORUS_r = (10.137, 10.137, 10.137), 6.0, 2.2
FIELD_ORIGIN = (-0.5, -0.5, -0.5)  # voxel (k, j, i) has its centre at (i, j, k): world coordinates are grid coordinates


def _grid(n):
    k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    return i, j, k


def sphere_distance(x, y, z, c=SPHERE_C, r=SPHERE_R):
    return np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def torus_distance(x, y, z):
    ring = np.sqrt((x - TORUS_C[0]) ** 2 + (y - TORUS_C[1]) ** 2) - TORUS_R
    return np.sqrt(ring ** 2 + (z - TORUS_C[2]) ** 2) - TORUS_r


@functools.lru_cache(maxsize=None)
def field(kind, n=FIELD_N):
    """(tsdf, weight) float32 [n, n, n] of the distance field in units of FIELD_TRUNC cells, clamped to [-1, 1]; the sphere and the
    torus are scaled with n, so that n = 96 is the same shape over many blocks"""
    i, j, k = _grid(n)
    s = n / FIELD_N
    d = (sphere_distance(i / s, j / s, k / s) if kind == "sphere" else torus_distance(i / s, j / s, k / s)) * s
    return np.clip(d / FIELD_TRUNC, -1.0, 1.0).astype(f32), np.ones((n, n, n), dtype=f32)


@functools.lru_cache(maxsize=None)
def field_ref(kind, n=FIELD_N, max_vertices=None, max_faces=None, slab=False, min_weight=0.5):
    tsdf, weight = field(kind, n)
    if slab:
        weight = weight.copy()
        k, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        weight[:, SLAB[0]:SLAB[1], :] *= ((i + 2 * k) % 3 == 0)[:, None, :]
    m = {}
    out = tr.extract_mesh(tsdf, weight, None, FIELD_ORIGIN, 1.0, min_weight=min_weight, max_vertices=max_vertices, max_faces=max_faces, margins=m)
    out["margins"] = m
    return out


# Rows j of the 20^3 sphere in which only the voxels with (i + 2 k) % 3 == 0 keep their weight: the mesh is open there.  A flat cut
# alone leaves no rim vertex (every edge in a face of a cell belongs to a tetrahedron of that cell); the voxels left inside the slab
# are joined by the x-z diagonals (i, k) - (i + 1, k + 1) alone, whose tetrahedra all have a corner without weight.
SLAB = (8, 11)


def check_topology(faces, nv, euler, closed=True):
    """faces [m, 3] below counts of a mesh of nv vertices: no degenerate face, every vertex used, every directed edge once, and for
    a closed surface every undirected edge in exactly two faces; V - E + F = euler"""
    faces = np.asarray(faces, dtype=np.int64)
    assert faces.min() >= 0 and faces.max() < nv
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    assert len(np.unique(faces)) == nv
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    codes = directed[:, 0] * nv + directed[:, 1]
    assert len(np.unique(codes)) == len(codes)  # consistent orientation: no directed edge twice
    und = np.sort(directed, axis=1)
    _, per_edge = np.unique(und[:, 0] * nv + und[:, 1], return_counts=True)
    if closed:
        assert (per_edge == 2).all()
    else:
        assert per_edge.max() <= 2
    assert nv - len(per_edge) + len(faces) == euler
    return per_edge


# The sphere's error bounds.  With L = sqrt(3) the longest edge and rho the distance to the centre, f = rho - R has
# |D^2 f| <= 1 / rho and |D^3 f| <= 3 / rho^2 (D^3 rho [u, v, w] = -((u.n)(Pv.Pw) + (v.n)(Pu.Pw) + (w.n)(Pu.Pv)) / rho^2, P = I - n n^T).
#   position  a crossing edge has both ends within L of the surface, so rho >= R - L on it, and linear interpolation of f along it
#             misses the zero by at most L^2 / 8 max|f''| = L^2 / (8 (R - L)) in f, which is a distance (|grad f| = 1)
#   normal    a central difference is off by at most |D^3 f| / 6 per component at rho >= R - L - 1 (its stencil reaches one cell
#             further), sqrt(3) times that as a vector; interpolating the gradient along the edge is off by at most
#             L^2 / 8 max|D^3 f| at rho >= R - L; the true normal at the vertex is grad f there, a unit vector wherever the vertex
#             lies, so the angle is at most asin of the sum
# and both get the float32 rounding of the stored field (2^-24 of 1, in units of FIELD_TRUNC cells) and of the outputs on top.
_L = np.sqrt(3.0)
SPHERE_POS_BOUND = _L ** 2 / (8.0 * (SPHERE_R - _L)) + 1e-5
SPHERE_NORMAL_BOUND = float(np.arcsin(np.sqrt(3.0) / 6.0 * 3.0 / (SPHERE_R - _L - 1.0) ** 2 + _L ** 2 / 8.0 * 3.0 / (SPHERE_R - _L) ** 2)) + 1e-4


def check_sphere_geometry(vertices, normals):
    v = np.asarray(vertices, dtype=np.float64)
    assert np.abs(sphere_distance(v[:, 0], v[:, 1], v[:, 2])).max() <= SPHERE_POS_BOUND
    true = (v - np.asarray(SPHERE_C)) / np.linalg.norm(v - np.asarray(SPHERE_C), axis=1, keepdims=True)
    n = np.asarray(normals, dtype=np.float64)
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    angle = np.arccos(np.clip((n * true).sum(axis=1), -1.0, 1.0))
    assert angle.max() <= SPHERE_NORMAL_BOUND
    return float(np.abs(sphere_distance(v[:, 0], v[:, 1], v[:, 2])).max()), float(angle.max())


# ------------------------------------------------------------------------------------------------------------ integration cases
SMALL_SEED, LARGE_SEED, GAUGE_SEED = 3, 5, 7
SMALL_DIMS, LARGE_DIMS = (24, 20, 16), (96, 80, 64)
FAR_SHIFT = (1e3, -2e3, 5e2)


def scene_case(V, H, W, dims, seed, weights=True, colors=True, shift=None, noise=0.004, view_valid=None, phase=0.0):
    """the two-plane scene seen by V cameras: depth = the true depth times (1 + noise N), 3 % of the cells without one (NaN, 0 or
    negative); depth_weight in (0.2, 1], 3 % of it 0 or NaN; images of random sizes and pixels.  The volume covers x in [-1.6, 1.6],
    y in [-2, 2], z in [2.6, 7.4] with cubic voxels; shift moves scene, cameras and volume together."""
    g = np.random.default_rng(seed)
    K, R, t = cameras_around(V, H, W, seed)
    if phase:  # other cameras of the same scene
        for v in range(V):
            phi = 2.0 * np.pi * v / V + 0.3 + phase
            R[v], t[v] = look_at([1.0 * np.cos(phi), 0.8 * np.sin(phi), 0.3 * np.sin(2.0 * phi)])
    depth = np.stack([true_depth(K[v], R[v], t[v], H, W)[0] for v in range(V)])
    depth = depth * (1.0 + noise * g.normal(size=depth.shape))
    bad = g.random(depth.shape)
    depth = np.where(bad < 0.01, np.nan, np.where(bad < 0.02, 0.0, np.where(bad < 0.03, -1.0, depth))).astype(f32)
    dw = None
    if weights:
        dw = g.uniform(0.2, 1.0, depth.shape)
        bad = g.random(depth.shape)
        dw = np.where(bad < 0.015, 0.0, np.where(bad < 0.03, np.nan, dw)).astype(f32)
    images = [g.integers(0, 256, (int(g.integers(20, 60)), int(g.integers(20, 60)), 3), dtype=np.uint8) for _ in range(V)] if colors else None
    nz, ny, nx = dims
    vs = max(3.2 / nx, 4.0 / ny, 4.8 / nz)
    origin = np.array([-0.5 * nx * vs, -0.5 * ny * vs, 5.0 - 0.5 * nz * vs])
    if shift is not None:
        shift = np.asarray(shift, dtype=np.float64)
        t = t - R @ shift
        origin = origin + shift
    return dict(depth=depth, depth_weight=dw, K=K, R=R, t=t, images=images, dims=dims, origin=origin, voxel_size=vs, trunc=3.0 * vs,
                max_weight=64.0, near=1e-6, view_valid=view_valid)


def run_ref(c, views=None, state=None, margins=None, **kw):
    """the restatement on the views `views` (default: all) of case c, from `state` (default: a fresh volume)"""
    sel = list(range(len(c["depth"]))) if views is None else list(views)
    tsdf, weight, color = state if state is not None else tr.fresh(c["dims"], c["images"] is not None)
    return tr.integrate(tsdf, weight, color, c["depth"][sel], c["K"][sel], c["R"][sel], c["t"][sel], c["origin"], c["voxel_size"], c["trunc"],
                        depth_weight=None if c["depth_weight"] is None else c["depth_weight"][sel],
                        images=None if c["images"] is None else [c["images"][v] for v in sel],
                        view_valid=None if c["view_valid"] is None else [c["view_valid"][v] for v in sel],
                        max_weight=kw.get("max_weight", c["max_weight"]), near=c["near"], margins=margins)


SMALL_VARIANTS = [(True, True, 64.0), (False, True, 64.0), (True, False, 64.0), (False, False, 64.0), (True, True, 1.25), (False, False, 2.0)]


@functools.lru_cache(maxsize=None)
def small_case(weights=True, colors=True):
    return scene_case(3, 24, 32, SMALL_DIMS, SMALL_SEED, weights=weights, colors=colors)


@functools.lru_cache(maxsize=None)
def small_ref(weights, colors, max_weight):
    m = {}
    out = run_ref(small_case(weights, colors), margins=m, max_weight=max_weight)
    return out, m


@functools.lru_cache(maxsize=None)
def large_case(far=False):
    return scene_case(8, 48, 64, LARGE_DIMS, LARGE_SEED, colors=False, shift=FAR_SHIFT if far else None,
                      view_valid=(1, 1, 0, 1, 1, 1, 1, 1) if far else None)


@functools.lru_cache(maxsize=None)
def large_ref(far=False):
    m = {}
    out = run_ref(large_case(far), margins=m)
    return out, m


RAGGED_VALID = (True, False, True)


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """three problems on one grid: an ordinary one, one that is not valid, one whose depth maps are empty"""
    cases = [scene_case(3, 24, 32, SMALL_DIMS, 20 + b, colors=False) for b in range(3)]
    cases[2]["depth"] = np.full_like(cases[2]["depth"], np.nan)
    return cases


@functools.lru_cache(maxsize=None)
def ragged_refs():
    out = []
    for b, c in enumerate(ragged_batch()):
        m = {}
        state = run_ref(c, margins=m) if RAGGED_VALID[b] else tr.fresh(c["dims"])  # a fresh volume has no valid voxel: an empty mesh
        mesh = tr.extract_mesh(state[0], state[1], None, c["origin"], c["voxel_size"], min_weight=0.1, margins=m)
        out.append((state, mesh, m))
    return out


# ----------------------------------------------------------------------------------------------------------------------- the chain
CHAIN_DIMS, CHAIN_TRUNC_VOXELS = (64, 64, 64), 4.0
CHAIN_DEPTH_NOISE = 1e-3  # relative: what the bounds assume of the fused depth maps, asserted in check_chain
CHAIN_WINDOW = 3          # pixels: a rendered depth is compared where the (2 * 3 + 1)^2 pixels around it see one surface


def surface_distance(X):
    """distance of world points [n, 3] to the nearer of the two surfaces AS SETS: the background plane, and the foreground rectangle
    with its border.  Inside the rectangle's prism this is depth_fusion_cases.plane_distance; beside it plane_distance knows only
    the background, 2 units away, although the wall that closes the volume behind the rectangle's silhouette stands a voxel or two
    from the rectangle's border - so there the distance to the border is what counts."""
    X = np.asarray(X, dtype=np.float64)
    d_bg = np.abs(X @ BG_N - BG_D)
    lateral = np.hypot(np.maximum(np.abs(X[:, 0]) - FG_X, 0.0), np.maximum(np.abs(X[:, 1]) - FG_Y, 0.0))
    d = np.minimum(d_bg, np.hypot(lateral, X[:, 2] - FG_Z))
    prism = lateral == 0
    assert np.array_equal(d[prism], plane_distance(X[prism]))
    return d


def check_chain(c, depth, voxel_size, vertices, rendered):
    """The mesh of the fused depth maps of depth_fusion_cases.chain_case: depth [V, H, W] the fused maps, vertices [n, 3] below
    counts, rendered [H, W] the vertices through render_points into view 0 with radius 1 and both passes off.

    Where a vertex can lie: it sits on an edge (at most sqrt(3) voxels long) one end of which has a negative mean, so some view
    saw that end behind its surface by at most trunc along the ray - at most trunc sec(a) in space, a the angle of the ray to the
    axis - of the surface point S that the CELL's centre ray hits, which is up to half a cell diagonal, sqrt(0.5) z / f, to the
    side of the voxel's own ray; and S is on a true surface up to the noise of the fused depth, CHAIN_DEPTH_NOISE z sec(a).  With
    tan(a) <= 0.5 sqrt(H^2 + W^2) / f the distance to the nearer surface is at most
        bound = (trunc_voxels sec(a) + sqrt(3)) voxels + (sqrt(0.5) / f + noise sec(a)) z_max.
    The distance is surface_distance: plane_distance inside the rectangle's prism, the distance to the rectangle beside it.

    The rendered depth of a pixel is that of the nearest vertex whose ray lies within 1.5 pixels of its centre.  That vertex is
    within `bound` of a point S of a true surface, which view 0 sees at most reach = 1.5 + bound f / z_min pixels from the pixel:
      - every rendered depth is at least the smallest true depth within `reach` pixels, less `bound`: nothing floats in front
      - where the pixels within CHAIN_WINDOW see the rectangle alone, nothing of the background can come in front of it, so the
        nearest vertex is the rectangle's: there a rendered depth must exist, and it is within bound / cos(b) of the plane's depth
        along the vertex's own ray, b the angle between ray and plane normal, which differs from the pixel's by at most `spread`,
        the plane's largest difference over the window; the fused depth adds its noise
      - the same holds on the background where all pixels within `reach` see the background.
    Returns the two measured maxima, in voxels."""
    H, W, V = c["H"], c["W"], c["V"]
    depth = np.asarray(depth, dtype=np.float64)
    truth = np.stack([c["truth"][v][0] for v in range(V)])
    have = np.isfinite(depth)
    assert have.mean() > 0.5 and (np.abs(depth[have] / truth[have] - 1.0) < CHAIN_DEPTH_NOISE).all()  # what the bound assumes
    vs = float(voxel_size)
    f = min(c["K_grid_exact"][v][0, 0] for v in range(V))
    sec = float(np.sqrt(1.0 + (0.5 * np.hypot(H, W) / f) ** 2))
    bound = (CHAIN_TRUNC_VOXELS * sec + np.sqrt(3.0)) * vs + (np.sqrt(0.5) / f + CHAIN_DEPTH_NOISE * sec) * float(depth[have].max())
    vertices = np.asarray(vertices, dtype=np.float64)
    dist = surface_distance(vertices)
    print(f"voxel {vs:.4f}: {len(vertices)} vertices within {dist.max() / vs:.3f} voxels of a surface (bound {bound / vs:.3f}), median {np.median(dist) / vs:.3f}")
    assert np.isfinite(vertices).all() and dist.max() <= bound
    Kg, zr = c["K_grid_exact"][0], np.asarray(rendered, dtype=np.float64)
    d0, label = c["truth"][0][0], c["truth"][0][1]
    reach = int(np.ceil(1.5 + bound * Kg[0, 0] / d0.min()))

    def window(radius, fn, start):
        """fn folded over the pixels within `radius`, the image's border repeated"""
        out, padded = start.copy(), lambda a: np.pad(a, radius, mode="edge")
        for dr in range(2 * radius + 1):
            for dc in range(2 * radius + 1):
                out = fn(out, dr, dc, padded)
        return out
    nearest = window(reach, lambda out, dr, dc, pad: np.minimum(out, pad(d0)[dr:dr + H, dc:dc + W]), d0)
    seen = np.isfinite(zr)
    assert seen.mean() > 0.5 and (zr[seen] >= nearest[seen] - bound).all()
    two_sided = np.zeros((H, W), dtype=bool)
    for lab, radius in ((1, CHAIN_WINDOW), (0, reach)):
        two_sided |= window(radius, lambda out, dr, dc, pad, lab=lab: out & (pad(label)[dr:dr + H, dc:dc + W] == lab), label == lab)
    spread = window(CHAIN_WINDOW, lambda out, dr, dc, pad: np.maximum(out, np.abs(pad(d0)[dr:dr + H, dc:dc + W] - d0)), np.zeros((H, W)))
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ray = np.stack([(cc - Kg[0, 2]) / Kg[0, 0], (rr - Kg[1, 2]) / Kg[1, 1], np.ones_like(cc)], axis=-1) @ c["R"][0]  # in the world
    cosb = np.abs(np.where(label == 1, ray[..., 2], ray @ BG_N)) / np.linalg.norm(ray, axis=-1)
    ok = two_sided & have[0]
    margin = bound / cosb + spread + CHAIN_DEPTH_NOISE * d0
    err = np.abs(zr - depth[0])
    assert ok.sum() >= 50 and seen[ok].all()
    print(f"{ok.sum()} of {H * W} pixels compared on both sides: |rendered - fused depth| at most {np.max(err[ok]) / vs:.3f} voxels, "
          f"{np.max(err[ok] / margin[ok]):.3f} of the margin; reach {reach} pixels")
    assert (err[ok] <= margin[ok]).all()
    return dist.max() / vs, np.max(err[ok]) / vs


def gpu_margins():
    """(name, margins) of every case that test_gpu_tsdf.py compares bit for bit"""
    m = {}
    c = hand_made()
    s = run_ref(c, margins=m)
    tr.extract_mesh(s[0], s[1], None, c["origin"], c["voxel_size"], min_weight=0.5, margins=m)
    yield "hand_made", m
    for w, col, mw in SMALL_VARIANTS:
        yield f"small {w} {col} {mw}", small_ref(w, col, mw)[1]
    for far in (False, True):
        yield f"large far={far}", large_ref(far)[1]
    for b, (_, _, m) in enumerate(ragged_refs()):
        yield f"ragged {b}", m
    for kind, n in (("sphere", 20), ("torus", 20), ("sphere", 96)):
        yield f"{kind} {n}", field_ref(kind, n)["margins"]
    yield "sphere slab", field_ref("sphere", 20, slab=True)["margins"]
