"""What the point-rendering tests share (test_cpu_point_render.py, test_gpu_point_render.py): the cases, chosen for where the
operator can go wrong and not for the size of the workload, and their restatements (tools/point_render_ref.py), computed once.
A case is a dict points [N, 3] f32, colors [N, 3] u8 or None, count, cameras [C, 3, 3] (output pixels), R [C, 3, 3], t [C, 3], H, W
and kw, the keywords of the call."""
import functools
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import point_render_ref as prr  # noqa: E402

f32 = np.float32
NAN = float("nan")
OFF = dict(occlusion_radius=0, fill_radius=0)  # both passes off


def ref(c, **kw):
    return prr.render(c["points"], c["cameras"], c["R"], c["t"], c["H"], c["W"], colors=c["colors"], count=c["count"], **dict(c["kw"], **kw))


# ---- the hand-made case: one camera at the origin looking along z, 8 x 8, K = [[2, 0, 1], [0, 2, -1]]: a row meant for the cell
# (r0, c0) at depth z is X = (((c0 + 0.5) - 1) / 2 z, ((r0 + 0.5) + 1) / 2 z, z) - every number dyadic, every division exact.
# radius 1 (3 x 3 splats), occlusion_radius 1 with count 3, fill_radius 1 with fill_min 6, near 0.5, far 10, count 13.
_HAND_ROWS = [          # (r0, c0, z)                                                                      covers (clipped)
    (2, 1, 3.0),        # 0  the cell of row 1 at another depth: loses everywhere
    (2, 1, 2.0),        # 1  near surface                                                                  rows 1-3, cols 0-2
    (2, 5, 2.0),        # 2  near surface                                                                  rows 1-3, cols 4-6
    (2, 5, 2.0),        # 3  the cell and the float32 depth of row 2: the lower row wins everywhere
    (0, 3, 2.0),        # 4  near surface, clipped at the top                                              rows 0-1, cols 2-4
    (4, 3, 2.0),        # 5  near surface                                                                  rows 3-5, cols 2-4
    (2, 3, 4.0),        # 6  far surface: rows 1-3, cols 2-4, of which only (2, 3) has no near row - the see-through pixel
    None,               # 7  behind the camera: (0.5, 0.5, -1)
    (6, 4, 12.0),       # 8  beyond far
    (6, 8, 2.0),        # 9  floor(u) = 8 = W: outside the frustum, the splat still reaches the border         rows 5-7, col 7
    (7, 0, 2.0),        # 10 clipped at the corner                                                         rows 6-7, cols 0-1
    None,               # 11 NaN
    (6, 9, 1.0),        # 12 floor(u) = 9 = W + radius: out of reach
    (6, 4, 1.0),        # 13 beyond count
]
HAND_KW = dict(radius=1, near=0.5, far=10.0, occlusion_radius=1, occlusion_rel=0.05, occlusion_count=3, fill_radius=1, fill_min=6,
               background=(9, 8, 7))
HAND_COUNT = 13
# What must come out.  Step 1, the row a pixel holds (every depth is 2 but F's 4; where near rows meet the lowest wins):
HAND_RAW_INDEX = [
    [-1, -1, 4, 4, 4, -1, -1, -1],
    [1, 1, 1, 4, 2, 2, 2, -1],
    [1, 1, 1, 6, 2, 2, 2, -1],
    [1, 1, 1, 5, 2, 2, 2, -1],
    [-1, -1, 5, 5, 5, -1, -1, -1],
    [-1, -1, 5, 5, 5, -1, -1, 9],
    [10, 10, -1, -1, -1, -1, -1, 9],
    [10, 10, -1, -1, -1, -1, -1, 9],
]
# Step 2: (2, 3) holds 4 > 2 * 1.05 with eight nearer neighbours - removed; nothing is nearer than any other pixel.  Step 3: (2, 3)
# has eight survivors around it and takes the smallest key among them, depth 2 of row 1; no empty pixel sees six survivors (the most
# is five, at (4, 1) and (4, 5)).  So the final index is the raw one with (2, 3) = 1, every depth is 2, mask 7 at (2, 3).
HAND_EXPECTED = {
    "index": [[1 if (r, c) == (2, 3) else v for c, v in enumerate(row)] for r, row in enumerate(HAND_RAW_INDEX)],
    "stats": (8, 37, 1, 1),  # rows 0-6 and 10 have their cell inside the image; 37 pixels hit
}


def check_hand_made(o):
    """o: the outputs as numpy arrays (the operator's or the restatement's)"""
    idx = np.asarray(HAND_EXPECTED["index"])
    have = idx >= 0
    assert np.array_equal(o["index"][0], idx), o["index"][0]
    assert np.array_equal(o["depth"][0], np.where(have, f32(2.0), f32(NAN)), equal_nan=True)
    mask = have.astype(np.uint8)
    mask[2, 3] = 7
    assert np.array_equal(o["mask"][0], mask)
    assert tuple(int(x) for x in o["stats"][0]) == HAND_EXPECTED["stats"]
    rows = np.arange(len(_HAND_ROWS))
    col = np.stack([10 * rows + 1, 10 * rows + 2, 10 * rows + 3], axis=1)
    assert np.array_equal(o["color"][0], np.where(have[..., None], col[np.where(have, idx, 0)], np.array(HAND_KW["background"])))


def hand_made():
    pts = np.zeros((len(_HAND_ROWS), 3), dtype=f32)
    for n, row in enumerate(_HAND_ROWS):
        if row is not None:
            r0, c0, z = row
            pts[n] = (((c0 + 0.5) - 1.0) / 2.0 * z, ((r0 + 0.5) + 1.0) / 2.0 * z, z)
    pts[7] = (0.5, 0.5, -1.0)
    pts[11] = NAN
    rows = np.arange(len(pts))
    colors = np.stack([10 * rows + 1, 10 * rows + 2, 10 * rows + 3], axis=1).astype(np.uint8)
    K = np.array([[[2.0, 0.0, 1.0], [0.0, 2.0, -1.0], [0.0, 0.0, 1.0]]])
    return {"points": pts, "colors": colors, "count": HAND_COUNT, "cameras": K, "R": np.eye(3)[None], "t": np.zeros((1, 3)), "H": 8, "W": 8,
            "kw": HAND_KW}


# ---- scenes: a dense far surface z = 6 + 0.3 x - 0.2 y that ends before the right border of the frame (the fill has an edge to
# grow at whatever the splat covers), behind a near one z = 3 + 0.1 x that covers part of the image with about one row per ten
# pixels; cameras turned about the point (0, 0, 5); then rows behind the cameras, rows with an infinite coordinate and, at the
# end, NaN padding
def _rot(ay, ax):
    cy, sy, cx, sx = np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
    return np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])


def scene(N, C, H, W, seed, with_colors=True):
    g = np.random.default_rng(seed)
    f = 0.9 * W * (1.0 + 0.05 * g.random())
    K = np.stack([np.array([[f * (1.0 + 0.02 * k), 0.0, W / 2.0 + 0.3 - 0.11 * k], [0.0, f * 1.03, H / 2.0 - 0.2 + 0.07 * k], [0.0, 0.0, 1.0]])
                  for k in range(C)])
    centre = np.array([0.0, 0.0, 5.0])
    R = np.stack([_rot(a, b) for a, b in zip((0.0, 0.12, -0.15, 0.07)[:C], (0.0, 0.05, 0.1, -0.04)[:C])])
    t = np.stack([centre - R[k] @ centre + np.array([0.02 * k, -0.03 * k, 0.1 * k]) for k in range(C)])
    n_pad, n_bad = N // 100, N // 100
    half_w, half_h = 0.75 * W / f * 6.0, 0.75 * H / f * 6.0  # 1.5 times the half-frame at the depth of the far surface
    near_px = (1.8 * f / 3.0) * (1.5 * f / 3.0)
    n_near = int(near_px / 10.0)
    n_far = N - n_pad - n_bad - n_near
    xf, yf = g.uniform(-half_w, 0.5 * half_w, n_far), g.uniform(-half_h, half_h, n_far)  # the right of the frame stays empty
    far = np.stack([xf, yf, 6.0 + 0.3 * xf - 0.2 * yf], axis=1)
    xn, yn = g.uniform(-1.2, 0.6, n_near), g.uniform(-0.8, 0.7, n_near)
    near = np.stack([xn, yn, 3.0 + 0.1 * xn], axis=1)
    bad = np.stack([g.uniform(-2, 2, n_bad), g.uniform(-2, 2, n_bad), g.uniform(-9.0, -0.5, n_bad)], axis=1)
    bad[::2, g.integers(0, 3)] = np.inf  # every other of them: an infinite coordinate instead
    body = np.concatenate([far, near, bad])[g.permutation(n_far + n_near + n_bad)]
    pts = np.concatenate([body, np.full((n_pad, 3), NAN)]).astype(f32)
    colors = g.integers(0, 256, (N, 3), dtype=np.uint8) if with_colors else None
    return {"points": pts, "colors": colors, "count": None, "cameras": K, "R": R, "t": t, "H": H, "W": W, "kw": {}}


# ---- random: N = 20 000 (79 blocks of rows), C = 3, 48 x 64 (12 blocks of pixels)
RANDOM_SEED = 41
FILTERS = {"off": dict(occlusion_radius=0), "o2c1": dict(occlusion_radius=2, occlusion_count=1), "o2c3": dict(occlusion_radius=2, occlusion_count=3)}
FILLS = {"off": dict(fill_radius=0), "f1m3": dict(fill_radius=1, fill_min=3)}
RANDOM_PARAMS = [(radius, flt, fil) for radius in (0, 1, 2) for flt in FILTERS for fil in FILLS]


def random_kw(radius, flt, fil):
    return dict(radius=radius, **FILTERS[flt], **FILLS[fil])


@functools.lru_cache(maxsize=None)
def random_case():
    return scene(20000, 3, 48, 64, RANDOM_SEED)


@functools.lru_cache(maxsize=None)
def random_ref(radius, flt, fil):
    return ref(random_case(), **random_kw(radius, flt, fil))


@functools.lru_cache(maxsize=None)
def random_cut(n=2000):
    """the first n rows of the random case"""
    c = random_case()
    return dict(c, points=c["points"][:n], colors=c["colors"][:n])


# ---- contention: 4 096 rows inside pixel (7, 9) of a 16 x 16 image; 64 of them share the smallest float32 depth, and they are not
# the lowest rows of the array
CONTENTION_SEED = 42
CONTENTION_PIXEL = (7, 9)


@functools.lru_cache(maxsize=None)
def contention_case():
    g = np.random.default_rng(CONTENTION_SEED)
    n = 4096
    z = g.uniform(2.0, 5.0, n)
    shared = np.sort(g.choice(np.arange(200, n), 64, replace=False))
    z[shared] = 1.5
    u, v = CONTENTION_PIXEL[1] + g.uniform(0.2, 0.8, n), CONTENTION_PIXEL[0] + g.uniform(0.2, 0.8, n)
    K = np.array([[[20.0, 0.0, 8.0], [0.0, 20.0, 8.0], [0.0, 0.0, 1.0]]])
    pts = np.stack([(u - 8.0) / 20.0 * z, (v - 8.0) / 20.0 * z, z], axis=1).astype(f32)
    return {"points": pts, "colors": None, "count": None, "cameras": K, "R": np.eye(3)[None], "t": np.zeros((1, 3)), "H": 16, "W": 16,
            "kw": dict(radius=0, **OFF), "shared": shared}


@functools.lru_cache(maxsize=None)
def contention_ref(radius=0):
    return ref(contention_case(), radius=radius)


# ---- large: 300 000 rows, C = 2, 200 x 320, with and without colours, the defaults of render_points
LARGE_SEED = 43


@functools.lru_cache(maxsize=None)
def large_case(with_colors=True):
    c = scene(300000, 2, 200, 320, LARGE_SEED)
    return c if with_colors else dict(c, colors=None)


@functools.lru_cache(maxsize=None)
def large_ref(with_colors=True):
    return ref(large_case(with_colors))


# ---- a ragged batch: B = 3 of N = 2 000, C = 2, 24 x 40, cameras per problem; the second problem is not valid
RAGGED_SEEDS = (44, 45, 46)
RAGGED_VALID = (1, 0, 1)
RAGGED_COUNTS = (1500, 0, 1100)  # and, in a second run, no counts at all: then `valid` alone empties the second problem


@functools.lru_cache(maxsize=None)
def ragged_batch():
    return [scene(2000, 2, 24, 40, s) for s in RAGGED_SEEDS]


@functools.lru_cache(maxsize=None)
def ragged_refs(with_counts=True):
    return [prr.render(c["points"], c["cameras"], c["R"], c["t"], c["H"], c["W"], colors=c["colors"],
                       count=RAGGED_COUNTS[b] if with_counts else None, valid=bool(RAGGED_VALID[b])) for b, c in enumerate(ragged_batch())]


# every (name, margins) the GPU file compares bit for bit: test_cpu_point_render.py asserts each margin is above 1e-9
def gpu_margins():
    yield "hand_made", ref(hand_made())["margins"]
    for p in RANDOM_PARAMS:
        yield "random %d %s %s" % p, random_ref(*p)["margins"]
    for radius in (0, 1):
        yield f"contention {radius}", contention_ref(radius)["margins"]
    yield "large", large_ref(True)["margins"]
    for wc in (True, False):
        for b, o in enumerate(ragged_refs(wc)):
            yield f"ragged {b} counts {wc}", o["margins"]
