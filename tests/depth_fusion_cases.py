"""What the depth-fusion tests share (test_cpu_depth_fusion.py, test_gpu_depth_fusion.py): a closed-form scene in numpy float64 - a
tilted background plane behind a smaller fronto-parallel foreground rectangle, V cameras around them, the true depth of a pixel
the nearest ray-plane hit, so some pixels are occluded in some views - and the cases built on it.  Operator cases are hypothesis
maps made directly (true depth + noise + planted outliers, flagged and zero-certainty slots); chain cases are ground-truth warps
(the hit projected into the other view, normalised) that go through triangulate_warp.  A hand-made V = 3, 2 x 3 case has its
expected outputs written out.  A case is a dict points [P, H, Wd, 3] f32, flags [P, H, Wd] u8, certainty [P, H, Wd] f32 or None,
pairs, cameras [V, 3, 3] (grid units), R [V, 3, 3], t [V, 3], symmetric."""
import functools
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import depth_fusion_ref as dfr  # noqa: E402
import triangulate_ref as trr  # noqa: E402

f32 = np.float32
NAN = float("nan")

# the scene: background plane n . X = n . (0, 0, 6), foreground rectangle |x| < 0.9, |y| < 0.6 at z = 4
BG_N = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
BG_D = float(BG_N @ np.array([0.0, 0.0, 6.0]))
FG_Z, FG_X, FG_Y = 4.0, 0.9, 0.6


def ref(c, **kw):
    kw.setdefault("symmetric", c["symmetric"])
    return dfr.fuse(c["points"], c["flags"], c["certainty"], c["pairs"], c["cameras"], c["R"], c["t"], **kw)


def look_at(centre, target=(0.0, 0.0, 5.0)):
    """(R, t) with x_cam = R X + t of a camera at `centre` whose axis points at `target`, x to the right, y down"""
    centre = np.asarray(centre, dtype=np.float64)
    z = np.asarray(target, dtype=np.float64) - centre
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ centre


def cameras_around(V, H, W, seed=0):
    """V cameras on an ellipse in front of the scene, looking at it; intrinsics in grid units with off-centre principal points"""
    g = np.random.default_rng(1000 + seed)
    K, R, t = np.zeros((V, 3, 3)), np.zeros((V, 3, 3)), np.zeros((V, 3))
    for v in range(V):
        phi = 2.0 * np.pi * v / V + 0.3
        R[v], t[v] = look_at([1.1 * np.cos(phi), 0.7 * np.sin(phi), 0.25 * np.cos(2.0 * phi)])
        f = 1.15 * max(H, W) * (1.0 + 0.05 * g.random())
        K[v] = [[f, 0.0, W / 2.0 + 0.31 * (g.random() - 0.5)], [0.0, f * 1.02, H / 2.0 + 0.27 * (g.random() - 0.5)], [0.0, 0.0, 1.0]]
    return K, R, t


def true_depth(K, R, t, H, W):
    """(depth [H, W], surface [H, W]: 1 foreground, 0 background, X [H, W, 3] the hit) of the cell centres of one view"""
    c, r = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d_cam = np.stack([(c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1], np.ones_like(c)], axis=-1)
    d_w = d_cam @ R  # R^T d
    C = -R.T @ t
    with np.errstate(all="ignore"):
        s_bg = (BG_D - BG_N @ C) / (d_w @ BG_N)
        s_fg = (FG_Z - C[2]) / d_w[..., 2]
        hit = C + s_fg[..., None] * d_w
        s_fg = np.where((np.abs(hit[..., 0]) < FG_X) & (np.abs(hit[..., 1]) < FG_Y) & (s_fg > 0), s_fg, np.inf)
        s_bg = np.where(s_bg > 0, s_bg, np.inf)
    depth = np.minimum(s_fg, s_bg)
    return depth, (s_fg < s_bg).astype(np.int64), C + depth[..., None] * d_w


def plane_distance(X):
    """distance of world points [n, 3] to the nearer of the two surfaces"""
    X = np.asarray(X, dtype=np.float64)
    d_bg = np.abs(X @ BG_N - BG_D)
    inside = (np.abs(X[:, 0]) < FG_X + 0.05) & (np.abs(X[:, 1]) < FG_Y + 0.05)
    return np.minimum(d_bg, np.where(inside, np.abs(X[:, 2] - FG_Z), np.inf))


def operator_case(V, H, W, pairs, seed, symmetric=True, noise=0.005, outliers=0.10, flagged=0.05, with_cert=True, usable=True):
    """hypothesis maps made directly: every slot is the true depth of its view times (1 + noise N(0, 1)); `outliers` of the slots
    are moved away by a factor, `flagged` get a flag byte, 2 % a zero certainty; half of the certainties are exactly 1.0, so ties
    of the summed weight are common.  usable False: every flag byte is set."""
    g = np.random.default_rng(seed)
    K, R, t = cameras_around(V, H, W, seed)
    truth = np.stack([true_depth(K[v], R[v], t[v], H, W)[0] for v in range(V)])
    P, Wd = len(pairs), (2 * W if symmetric else W)
    z = np.zeros((P, H, Wd))
    for p, (i, j) in enumerate(pairs):
        z[p, :, :W] = truth[i]
        if symmetric:
            z[p, :, W:] = truth[j]
    z = z * (1.0 + noise * g.standard_normal(z.shape))
    out = g.random(z.shape) < outliers
    factor = np.where(g.random(z.shape) < 0.5, g.uniform(0.4, 0.8, z.shape), g.uniform(1.25, 2.0, z.shape))
    z = np.where(out, z * factor, z)
    points = np.full((P, H, Wd, 3), 7.0, dtype=f32)  # x and y are never read
    points[..., 2] = z.astype(f32)
    flags = np.where(g.random(z.shape) < flagged, g.choice([2, 4, 8, 36], size=z.shape), 0).astype(np.uint8)
    if not usable:
        flags[:] = 4
    cert = np.where(g.random(z.shape) < 0.5, 1.0, g.uniform(0.2, 1.0, z.shape))
    cert = np.where(g.random(z.shape) < 0.02, 0.0, cert).astype(f32)
    return {"points": points, "flags": flags, "certainty": cert if with_cert else None, "pairs": list(pairs), "cameras": K, "R": R, "t": t,
            "symmetric": symmetric, "V": V, "H": H, "W": W, "truth": truth, "planted": out}


# ---- the random case of the issue: V = 4, grid 24 x 40 (Wd = 80 is no multiple of the wave), 6 pairs - (2, 0) reversed, (1, 3) in both orders
RANDOM_PAIRS = [(0, 1), (2, 0), (0, 3), (1, 2), (1, 3), (3, 1)]
RANDOM_SEED = 11
RANDOM_PARAMS = [(rel, ms, mc, dd) for rel in (0.01, 0.05) for ms in (1, 2, 3) for mc in (0, 1, 2) for dd in (0, 1)]


@functools.lru_cache(maxsize=None)
def random_case(symmetric=True, with_cert=True):
    return operator_case(4, 24, 40, RANDOM_PAIRS, RANDOM_SEED, symmetric=symmetric, with_cert=with_cert)


@functools.lru_cache(maxsize=None)
def random_ref(rel, ms, mc, dd, symmetric=True, with_cert=True):
    return ref(random_case(symmetric, with_cert), rel_thresh=rel, min_support=ms, min_consistent=mc, dedupe=bool(dd))


# ---- V = 3 at 160 x 200: 125 blocks a view, the scan crosses 375
LARGE_SEED = 12


@functools.lru_cache(maxsize=None)
def large_case():
    return operator_case(3, 160, 200, [(0, 1), (0, 2), (1, 2)], LARGE_SEED)


@functools.lru_cache(maxsize=None)
def large_ref(max_points=None):
    return ref(large_case(), max_points=max_points)


# ---- V = 8 at 184 x 180: 130 blocks a view, 1040 in all - the scan kernel's 1024 threads take two block counts each, the last ones none.
# A chain of pairs joins the views, so the end views have one slot a pixel: min_support = 1
WIDE_SEED = 19  # 18 puts a decision within 1.4e-11 of its threshold
WIDE_PAIRS = [(v, v + 1) for v in range(7)]
WIDE_CUT = 20000


@functools.lru_cache(maxsize=None)
def wide_case():
    return operator_case(8, 184, 180, WIDE_PAIRS, WIDE_SEED)


@functools.lru_cache(maxsize=None)
def wide_ref(max_points=None):
    return ref(wide_case(), min_support=1, max_points=max_points)


# ---- a ragged batch of 3 on the random shape: a problem that is not valid, one with a view switched off, one without a usable slot
RAGGED_SEEDS = (13, 14, 15)
RAGGED_VALID = (False, True, True)
RAGGED_VIEW_VALID = ((True, True, True, True), (True, False, True, True), (True, True, True, True))


@functools.lru_cache(maxsize=None)
def ragged_batch():
    return [operator_case(4, 24, 40, RANDOM_PAIRS, s, usable=(b != 2)) for b, s in enumerate(RAGGED_SEEDS)]


@functools.lru_cache(maxsize=None)
def ragged_refs():
    return [ref(c, min_support=1, valid=RAGGED_VALID[b], view_valid=RAGGED_VIEW_VALID[b]) for b, c in enumerate(ragged_batch())]


# ---- colours: V = 2 on a 20 x 28 grid with images of 50 x 70 and 33 x 91 pixels
COLOR_SEED = 16
COLOR_SIZES = [(50, 70), (33, 91)]


@functools.lru_cache(maxsize=None)
def color_case():
    c = operator_case(2, 20, 28, [(0, 1)], COLOR_SEED, outliers=0.0, flagged=0.02)
    g = np.random.default_rng(COLOR_SEED)
    c["images"] = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in COLOR_SIZES]
    return c


@functools.lru_cache(maxsize=None)
def color_ref():
    c = color_case()
    return ref(c, min_support=1, images=c["images"])


# ---- the hand-made case: V = 3, grid 2 x 3, every pair in both orders (4 slots a view), all rotations the identity
# View v sits at (b_v, 0, 0) and looks along z: a point at depth z of pixel (r, c) of view v lies, on the grid of view u, at
#   g_x = c + (cx_u - cx_v) + 4 (b_v - b_u) / z,   g_y = r + (cy_u - cy_v)
HAND_PAIRS = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]
HAND_B = (0.0, 0.25, -0.35)
HAND_CX = (1.5, 1.6, 1.35)
HAND_CY = (1.0, 1.25, 0.75)
HAND_KW = dict(rel_thresh=0.01, min_support=2, min_consistent=1, max_violations=0, dedupe=True)
# (view, r, c) -> the four slots (z, w, flag) of the pixel in slot order; every other slot is (4, 1, 0): the plane z = 4
_HAND_SLOTS = {
    (0, 0, 0): [(4.0, 1.0, 0), (4.02, 1.0, 0), (6.0, 1.0, 0), (4.0, 0.0, 0)],    # 2 against 1, the fourth has no certainty: mean 4.01
    (0, 0, 1): [(5.0, 0.5, 0), (5.0, 0.5, 0), (4.0, 0.75, 0), (4.0, 0.75, 0)],   # n = 2 twice: the weight 1.5 beats 1.0 of the lower slots -> 4
    (0, 0, 2): [(4.0, 0.5, 0), (4.0, 0.5, 0), (5.0, 0.5, 0), (5.0, 0.5, 0)],     # a full tie: the lower slot -> 4, weight 1
    (2, 1, 2): [(4.0, 1.0, 0), (5.0, 1.0, 0), (6.0, 1.0, 0), (4.0, 1.0, 4)],     # below min_support: best n = 1, no depth
    (1, 1, 1): [(2.0, 1.0, 0), (2.0, 1.0, 0), (2.0, 1.0, 0), (2.0, 1.0, 0)],     # floats in front of what view 0 sees
    (2, 0, 2): [(8.0, 1.0, 0), (8.0, 1.0, 0), (NAN, 1.0, 0), (-1.0, 1.0, 0)],    # behind what views 0 and 1 see; NaN and z < 0 are not usable
}
# What must come out, pixel by pixel (g is the position on the other view's grid by the formula above):
#   view 0 (1, 0): in view 2 at g = (0.2, 0.75), four neighbours at 4 -> seen by 2, kept, emitted first: X = (-1, 0.5, 4); in view 1
#                  g_y = 1.25 leaves the 2 x 2 neighbourhoods.  Row 0 of view 0 leaves view 2 (g_y = -0.25); in view 1 its neighbourhoods
#                  hold the 2 of (1, 1): the depth there is below 4, e > rel - occluded, neither bit.  (1, 1), (1, 2): a NaN neighbour / outside.
#   view 1 (1, 0): in view 0 at (0.15, 0.75) over 4.01, 4, 4, 4: e = -5.3e-4 -> seen by 0; in view 2 at (0.35, 0.5) -> seen by 2: seen = 5;
#                  the pixel of view 0 nearest (0.15, 0.75) is (1, 0), which is kept -> duplicate, state 3.
#   view 1 (1, 1): z = 2 lands in view 0 at (1.4, 0.75) over four 4s: e = -0.5 -> violated by 0; in view 2 a neighbour has no depth.
#   view 1 row 0 and (1, 2): outside both other grids -> seen 0, not kept.
#   view 2 (0, 1): in view 0 at (0.8, 0.25) over 4.01, 4, 4, 4: e = -3.7e-4 -> seen by 0, kept; nearest pixel (0, 1) of view 0 is not
#                  kept -> emitted second: X = (-0.2, -0.25, 4).  In view 1 the 2 of (1, 1) is a neighbour: occluded there.
#   view 2 (0, 2): z = 8 lands in view 0 at (1.975, 0.25) over four 4s: e = +1 -> occluded, neither bit; likewise in view 1: not kept.
HAND_EXPECTED = {
    "depth": [[[f32(4.01), 4.0, 4.0], [4.0, 4.0, 4.0]], [[4.0, 4.0, 4.0], [4.0, 2.0, 4.0]], [[4.0, 4.0, 8.0], [4.0, 4.0, NAN]]],
    "weight": [[[2.0, 1.5, 1.0], [4.0, 4.0, 4.0]], [[4.0, 4.0, 4.0], [4.0, 4.0, 4.0]], [[4.0, 4.0, 2.0], [4.0, 4.0, 0.0]]],
    "support": [[[2, 2, 2], [4, 4, 4]], [[4, 4, 4], [4, 4, 4]], [[4, 4, 2], [4, 4, 1]]],
    "seen": [[[0, 0, 0], [4, 0, 0]], [[0, 0, 0], [5, 0, 0]], [[0, 1, 0], [0, 0, 0]]],
    "violated": [[[0, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, 1, 0]], [[0, 0, 0], [0, 0, 0]]],
    "state": [[[0, 0, 0], [1, 0, 0]], [[0, 0, 0], [3, 0, 0]], [[0, 1, 0], [0, 0, 0]]],
    "source": [[0, 3], [2, 1]],                                # emission order: (view, pixel index)
    "points": [[-1.0, 0.5, 4.0], [f32(-0.2), -0.25, 4.0]],
    "cloud_weight": [4.0, 4.0],
    "total": 2,
    "stats": (18, 17, 3, 1, 2, 1, 0, 0),
    "source_without_dedupe": [[0, 3], [1, 3], [2, 1]],
}


def check_hand_made(o, dedupe=True):
    """o: the outputs as numpy arrays (the operator's or the restatement's), max_points = 4"""
    e = HAND_EXPECTED
    for k in ("depth", "weight"):
        assert np.array_equal(np.asarray(o[k], dtype=f32), np.asarray(e[k], dtype=f32), equal_nan=True), k
    for k in ("support", "seen", "violated"):
        assert np.array_equal(o[k], np.asarray(e[k])), k
    state = np.asarray(e["state"])
    src = e["source"] if dedupe else e["source_without_dedupe"]
    n = len(src)
    assert np.array_equal(o["state"], state if dedupe else state & 1)
    assert int(o["total"]) == n and int(o["count"]) == n and np.array_equal(o["source"][:n], src) and (o["source"][n:] == -1).all()
    if dedupe:
        assert np.array_equal(np.asarray(o["points"][:n], dtype=f32), np.asarray(e["points"], dtype=f32)) and tuple(o["stats"]) == e["stats"]
        assert np.array_equal(o["cloud_weight"][:n], e["cloud_weight"])
    assert np.isnan(o["points"][n:]).all() and not o["cloud_weight"][n:].any()


def hand_made():
    V, H, W = 3, 2, 3
    K = np.array([[[4.0, 0.0, HAND_CX[v]], [0.0, 4.0, HAND_CY[v]], [0.0, 0.0, 1.0]] for v in range(V)])
    R = np.stack([np.eye(3)] * V)
    t = np.array([[-HAND_B[v], 0.0, 0.0] for v in range(V)])
    P = len(HAND_PAIRS)
    points = np.full((P, H, 2 * W, 3), 7.0, dtype=f32)
    points[..., 2] = 4.0
    flags = np.zeros((P, H, 2 * W), dtype=np.uint8)
    cert = np.ones((P, H, 2 * W), dtype=f32)
    slots = dfr.slots_of(HAND_PAIRS, V, True)
    for (v, r, c), rows in _HAND_SLOTS.items():
        for (p, half), (z, w, f) in zip(slots[v], rows):
            points[p, r, half * W + c, 2], cert[p, r, half * W + c], flags[p, r, half * W + c] = z, w, f
    return {"points": points, "flags": flags, "certainty": cert, "pairs": HAND_PAIRS, "cameras": K, "R": R, "t": t, "symmetric": True,
            "V": V, "H": H, "W": W}


# ---- chain cases: ground-truth warps of the scene for images of mixed sizes
CHAIN_SEED = 17
CHAIN_SIZES = [(96, 128), (120, 150), (90, 140), (128, 128)]
CHAIN_PAIRS = [(a, b) for a in range(4) for b in range(a + 1, 4)]
CHAIN_GRID = (32, 44)


@functools.lru_cache(maxsize=None)
def chain_case():
    """warp [P, H, 2W, 4] f32 normalised and certainty [P, H, 2W] f32 (1 where the hit is visible inside the other image, else 0),
    image intrinsics K_img for CHAIN_SIZES, poses"""
    V, (H, W) = len(CHAIN_SIZES), CHAIN_GRID
    Kg, R, t = cameras_around(V, H, W, CHAIN_SEED)
    K_img = Kg.copy()
    for v, (h_img, w_img) in enumerate(CHAIN_SIZES):
        K_img[v, 0] *= w_img / W
        K_img[v, 1] *= h_img / H
    K_grid = np.stack([K_img[v] * np.array([[W / w_img], [H / h_img], [1.0]]) for v, (h_img, w_img) in enumerate(CHAIN_SIZES)])
    c, r = np.meshgrid((np.arange(W) + 0.5) / W * 2.0 - 1.0, (np.arange(H) + 0.5) / H * 2.0 - 1.0)
    own = np.stack([c, r], axis=-1)
    truth = [true_depth(K_grid[v], R[v], t[v], H, W) for v in range(V)]
    warp = np.zeros((len(CHAIN_PAIRS), H, 2 * W, 4))
    cert = np.zeros((len(CHAIN_PAIRS), H, 2 * W))
    for p, (i, j) in enumerate(CHAIN_PAIRS):
        for half, (a, b) in enumerate(((i, j), (j, i))):
            X = truth[a][2]
            y = X @ R[b].T + t[b]
            g = np.stack([K_grid[b][0, 0] * y[..., 0] / y[..., 2] + K_grid[b][0, 2], K_grid[b][1, 1] * y[..., 1] / y[..., 2] + K_grid[b][1, 2]], -1)
            other = np.stack([g[..., 0] / W * 2.0 - 1.0, g[..., 1] / H * 2.0 - 1.0], axis=-1)
            # visible in b: inside its image and not behind the surface b sees there (the foreground hides part of the background)
            db, _, _ = true_depth(K_grid[b], R[b], t[b], H, W)
            xi, yi = np.clip(np.floor(g[..., 0]), 0, W - 1).astype(int), np.clip(np.floor(g[..., 1]), 0, H - 1).astype(int)
            vis = (np.abs(other) < 1.0).all(axis=-1) & (y[..., 2] > 0) & (y[..., 2] < db[yi, xi] * 1.05)
            sl = np.s_[p, :, half * W:(half + 1) * W]
            warp[sl] = np.concatenate([own, other] if half == 0 else [other, own], axis=-1)
            cert[sl] = vis
    return {"warp": warp.astype(f32), "certainty": cert.astype(f32), "pairs": CHAIN_PAIRS, "K": K_img, "R": R, "t": t, "sizes": CHAIN_SIZES,
            "V": V, "H": H, "W": W, "truth": truth, "K_grid_exact": K_grid}


def chain_ref(c, **kw):
    """the chain of restatements: K to the grid, relative poses, triangulate_ref over the pairs, depth_fusion_ref"""
    H, W, V = c["H"], c["W"], c["V"]
    K_grid = np.stack([c["K"][v] * np.array([[W / int(w_img)], [H / int(h_img)], [1.0]]) for v, (h_img, w_img) in enumerate(c["sizes"])])
    R_ij, t_ij = dfr.relative_poses(c["R"], c["t"], c["pairs"])
    tri_kw = {k: kw.pop(k) for k in ("max_depth", "max_reproj", "min_parallax", "min_certainty") if k in kw}
    points, flags = [], []
    for p, (i, j) in enumerate(c["pairs"]):
        o = trr.triangulate(c["warp"][p].reshape(-1, 4), R_ij[p], t_ij[p], K_grid[i], K_grid[j], certainty=c["certainty"][p].reshape(-1),
                            coords=1, sizes=(W, H, W, H), sym_w=W, **tri_kw)
        points.append(o["points"].astype(f32).reshape(H, 2 * W, 3))
        flags.append(o["flags"].reshape(H, 2 * W))
    out = dfr.fuse(np.stack(points), np.stack(flags), c["certainty"], c["pairs"], K_grid, c["R"], c["t"], symmetric=True, **kw)
    out["tri_points"], out["tri_flags"] = np.stack(points), np.stack(flags)
    return out


@functools.lru_cache(maxsize=None)
def chain_ref_default():
    return chain_ref(chain_case(), min_certainty=0.5)


# every (name, margin) the GPU file compares bit for bit: test_cpu_depth_fusion.py asserts each margin is above 1e-9
def gpu_margins():
    yield "hand_made", ref(hand_made(), **HAND_KW)["margin"]
    for rel, ms, mc, dd in RANDOM_PARAMS:
        yield f"random {rel} {ms} {mc} {dd}", random_ref(rel, ms, mc, dd)["margin"]
    yield "random without certainty", random_ref(0.01, 2, 1, 1, True, False)["margin"]
    yield "random not symmetric", random_ref(0.01, 2, 1, 1, False, True)["margin"]
    yield "large", large_ref()["margin"]
    yield "wide", wide_ref()["margin"]
    for b, o in enumerate(ragged_refs()):
        yield f"ragged {b}", o["margin"]
    yield "colours", color_ref()["margin"]
    yield "chain", chain_ref_default()["margin"]
