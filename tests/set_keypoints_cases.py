"""What the detector-free keypoint tests share (test_cpu_set_keypoints.py, test_gpu_set_keypoints.py): the inputs of
roma_amd.keypoints_from_matches - a hand-made case with its expected output written out, seeded random cases, a large grid, a
scene whose pairwise matches must join into tracks - and the numpy chain `reconstruct_views` is held against, for arbitrary
keypoints.  A case is a dict matches [P, N, 4] f32 (normalised), certainty [P, N] f32, counts [P] int32, pairs, V, sizes [(H, W)]."""
import functools
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import set_keypoints_ref as skr  # noqa: E402
from views_cases import CONF, NORM_THR, THR, apr, br, pose_errors, prr, tkr, tvr, views_scene  # noqa: E402,F401

f32 = np.float32
ALL4 = [(a, b) for a in range(4) for b in range(a + 1, 4)]


def normalised(px, size):
    """pixels -> normalised coordinates, float32: the inverse of the operator's step 1 up to its rounding"""
    return (2.0 * np.asarray(px, np.float64) / size - 1.0).astype(f32)


def ref(c, **kw):
    return skr.keypoints_from_matches(c["matches"], c["certainty"], c["pairs"], c["V"], c["sizes"], counts=c["counts"], **kw)


# ---- hand-made: V = 3, sizes (5, 7), (4, 4), (6, 3), cell 2 (partial last cells), P = 3, N = 8
NAN = float("nan")
# rows (xA, yA, xB, yB, c) in PIXELS; "L" / "R": the normalised coordinate is exactly -1 / +1 (pixel 0: valid; pixel W: invalid)
_HAND_ROWS = [
    [  # pair (0, 1), all 8 rows read
        (0.5, 0.5, 0.5, 0.5, 1.0),    # 0 the triangle's first edge
        (1.0, 1.0, 3.5, 0.5, 1.0),    # 1 A in row 0's cell with the same certainty: the lower ordinal wins the cell; loses one_to_one to row 0
        ("L", 4.5, 0.5, 3.5, 0.5),    # 2 x = -1: pixel 0, valid; the partial last cell row of view 0
        ("R", 0.5, 0.5, 0.5, 1.0),    # 3 x = +1: pixel W, invalid
        (NAN, 0.5, 0.5, 0.5, 1.0),    # 4 NaN
        (2.5, 0.5, 2.5, 0.5, 0.0),    # 5 c = 0
        (6.5, 0.5, 3.5, 3.5, 0.2),    # 6 the partial last cell column of view 0; B loses its cell to row 7 and one_to_one with it
        (3.9, 2.5, 2.5, 2.5, 0.5),    # 7 left of the border x = 4 of view 0: pair (0, 2) row 1 lies right of it
    ],
    [  # pair (1, 2), 7 rows read
        (0.75, 0.5, 0.5, 0.5, 1.0),   # 0 A lands in the cell pair (0, 1) row 0 holds: two pairs in one cell, the earlier ordinal stays
        (3.5, 0.5, 2.75, 1.5, 0.5),   # 1
        (0.5, 3.5, 0.5, 5.5, 0.5),    # 2
        (2.5, 2.5, 0.5, 3.0, 0.2),    # 3
        (0.5, 0.5, 0.5, "R", 1.0),    # 4 y = +1: pixel H, invalid
        (0.5, 0.5, 0.5, 0.5, NAN),    # 5 certainty NaN
        (0.5, 0.5, 0.5, 0.5, -0.5),   # 6 certainty below 0
        (3.5, 3.5, 2.5, 5.5, 1.0),    # 7 beyond counts: would add keypoints if it were read
    ],
    [  # pair (0, 2), 6 rows read
        (0.5, 0.5, 0.5, 0.5, 1.0),    # 0 closes the triangle
        (4.1, 2.5, 0.5, 3.0, 0.5),    # 1 right of the border: suppressed by pair (0, 1) row 7's endpoint 0.2 px away and assigned to it
        (6.5, 0.5, 2.75, 1.5, 0.2),   # 2
        (2.5, 4.5, 0.5, 5.5, 0.5),    # 3
        (0.5, NAN, 0.5, 0.5, 1.0),    # 4 NaN
        (5.0, 4.5, 2.5, 4.5, 0.2),    # 5
        (1.0, 1.0, 2.5, 0.5, 1.0),    # 6 beyond counts
        (3.0, 3.0, 1.0, 1.0, 1.0),    # 7 beyond counts
    ],
]
HAND_SIZES = [(5, 7), (4, 4), (6, 3)]
HAND_PAIRS = [(0, 1), (1, 2), (0, 2)]


def hand_made():
    m, c = np.zeros((3, 8, 4), f32), np.zeros((3, 8), f32)
    for p, rows in enumerate(_HAND_ROWS):
        for n, row in enumerate(rows):
            for k in range(4):
                H, W = HAND_SIZES[HAND_PAIRS[p][k // 2]]
                v = row[k]
                m[p, n, k] = {"L": -1.0, "R": 1.0}[v] if isinstance(v, str) else normalised(v, W if k % 2 == 0 else H)
            c[p, n] = row[4]
    return dict(matches=m, certainty=c, counts=np.array([8, 7, 6], np.int32), pairs=HAND_PAIRS, V=3, sizes=HAND_SIZES)


# expected output for cell = 2, max_kpts = 8, one_to_one: radius -> (keypoints per view in pixels, scores, inds, kept, info)
_X = (-1, -1)
HAND_EXPECTED = {
    2.0: dict(
        kpts=[[(0.5, 0.5), (6.5, 0.5), (3.9, 2.5), (0.0, 4.5), (2.5, 4.5), (5.0, 4.5)],
              [(0.5, 0.5), (3.5, 0.5), (0.5, 3.5), (2.5, 2.5)],
              [(0.5, 0.5), (2.75, 1.5), (0.5, 3.0), (0.5, 5.5), (2.5, 4.5)]],
        score=[[1.0, 0.2, 0.5, 0.5, 0.5, 0.2], [1.0, 1.0, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5, 0.2]],
        inds=[[(0, 0), _X, (3, 2), _X, _X, _X, _X, (2, 3)],
              [(0, 0), (1, 1), (2, 3), (3, 2), _X, _X, _X, _X],
              [(0, 0), (2, 2), (1, 1), (4, 3), _X, (5, 4), _X, _X]],
        kept=[3, 4, 5], info=(21, 7, 0, 2, 12, 1)),
    0.0: dict(
        kpts=[[(0.5, 0.5), (6.5, 0.5), (3.9, 2.5), (4.1, 2.5), (0.0, 4.5), (2.5, 4.5), (5.0, 4.5)],
              [(0.5, 0.5), (3.5, 0.5), (0.5, 3.5), (2.5, 2.5)],
              [(0.5, 0.5), (2.75, 1.5), (0.5, 3.0), (0.5, 5.5), (2.5, 4.5)]],
        score=[[1.0, 0.2, 0.5, 0.5, 0.5, 0.5, 0.2], [1.0, 1.0, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5, 0.2]],
        inds=[[(0, 0), _X, (4, 2), _X, _X, _X, _X, (2, 3)],
              [(0, 0), (1, 1), (2, 3), (3, 2), _X, _X, _X, _X],
              [(0, 0), (3, 2), (1, 1), (5, 3), _X, (6, 4), _X, _X]],
        kept=[3, 4, 5], info=(21, 7, 0, 2, 12, 0)),
}


def check_hand_made(o, radius):
    """o: a dict of numpy arrays as tools/set_keypoints_ref.py returns it, for hand_made() at cell 2, max_kpts 8"""
    e = HAND_EXPECTED[radius]
    for v in range(3):
        n = len(e["kpts"][v])
        assert o["num_kpts"][v] == n and o["total"][v] == n
        assert np.abs(o["kpts"][v][:n] - np.array(e["kpts"][v], np.float32)).max() < 1e-5  # the rounding of pixel -> normalised -> pixel
        assert np.array_equal(o["score"][v][:n], np.array(e["score"][v], np.float32))
        assert np.isnan(o["kpts"][v][n:]).all() and not o["score"][v][n:].any()
    assert np.array_equal(o["inds"], np.array(e["inds"], np.int32))
    assert o["kept"].tolist() == e["kept"] and tuple(int(i) for i in o["info"]) == e["info"]


# ---- random: about 150 scene centres per view, +-0.6 px of jitter per pair, so that cells collide and straddle
RANDOM_SIZES = [(48, 64), (37, 53), (64, 48), (50, 50)]
RANDOM_COUNTS = (600, 599, 1, 0, 257, 64)


@functools.lru_cache(maxsize=None)
def random_case(seed=0, N=600, counts=RANDOM_COUNTS, centres=150, jitter=0.6):
    g = np.random.default_rng(seed)
    V, P = 4, len(ALL4)
    where = [np.stack([g.uniform(0, W, centres), g.uniform(0, H, centres)], axis=1) for H, W in RANDOM_SIZES]  # (x, y) per view
    m, c = np.zeros((P, N, 4), f32), np.zeros((P, N), f32)
    for p, (a, b) in enumerate(ALL4):
        pick = g.integers(0, centres, N)
        for side, v in enumerate((a, b)):
            H, W = RANDOM_SIZES[v]
            px = where[v][pick] + g.uniform(-jitter, jitter, (N, 2))
            m[p, :, 2 * side], m[p, :, 2 * side + 1] = normalised(px[:, 0], W), normalised(px[:, 1], H)
        c[p] = np.where(g.random(N) < 0.5, 1.0, g.uniform(0.01, 0.99, N)).astype(f32)
        # 2 % of the rows invalid in each way: outside, not finite, certainty 0, certainty NaN or negative
        kind = g.random(N)
        m[p, kind < 0.02, g.integers(0, 4)] = f32(1.0) + f32(g.uniform(0, 0.5))
        m[p, (kind >= 0.02) & (kind < 0.04), g.integers(0, 4)] = np.nan
        c[p, (kind >= 0.04) & (kind < 0.06)] = 0.0
        c[p, (kind >= 0.06) & (kind < 0.07)] = np.nan
        c[p, (kind >= 0.07) & (kind < 0.08)] = -0.25
    return dict(matches=m, certainty=c, counts=np.asarray(counts, np.int32), pairs=ALL4, V=V, sizes=RANDOM_SIZES)


RANDOM_PARAMS = [(cell, radius, K, o2o) for cell in (1, 2, 3) for radius in (0.0, cell / 2, float(cell)) for K in (4096, 100) for o2o in (0, 1)]


# ---- large grid: V = 3 at 864 x 1152 with cell 1: about 10^6 cells per view, the scan crosses many workgroups
LARGE_SIZES = [(864, 1152)] * 3
LARGE_PAIRS = [(0, 1), (1, 2), (0, 2)]


@functools.lru_cache(maxsize=None)
def large_case(seed=1, N=5000):
    g = np.random.default_rng(seed)
    H, W = LARGE_SIZES[0]
    m = np.stack([normalised(g.uniform(0, W, (3, N)), W), normalised(g.uniform(0, H, (3, N)), H),
                  normalised(g.uniform(0, W, (3, N)), W), normalised(g.uniform(0, H, (3, N)), H)], axis=-1)
    c = np.where(g.random((3, N)) < 0.5, 1.0, g.uniform(0.01, 0.99, (3, N))).astype(f32)
    # keypoints in the first and in the last cell of every grid
    m[:, 0], c[:, 0] = [normalised(0.5, W), normalised(0.5, H)] * 2, 1.0
    m[:, 1], c[:, 1] = [normalised(W - 0.5, W), normalised(H - 0.5, H)] * 2, 1.0
    return dict(matches=m.astype(f32), certainty=c, counts=np.array([N, N - 1, N], np.int32), pairs=LARGE_PAIRS, V=3, sizes=LARGE_SIZES)


# ---- ragged batch: three problems of the random shape, different counts, one without a valid row
def ragged_batch():
    a = random_case(0)
    b = dict(random_case(1), counts=np.array([5, 600, 300, 17, 0, 600], np.int32))
    c = dict(random_case(2))
    c["certainty"] = np.zeros_like(c["certainty"])  # no valid row at all
    c["counts"] = np.full(6, 600, np.int32)
    return [a, b, c]


# ---- a scene: views_scene(5, False) shifted to start at 0, its pairwise matches jittered independently
SCENE_JITTER, SCENE_SEED = 0.25, 0


@functools.lru_cache(maxsize=None)
def scene_case(seed=SCENE_SEED, jitter=SCENE_JITTER):
    """(case, scene): every pair's rows are the points seen in both views, each endpoint jittered by +-jitter px on its own,
    certainties from {1, 0.5, 0.2}; the scene's kpts and camera matrices are shifted with the window"""
    s = views_scene(5, False)
    kp = s["kpts"].astype(np.float64)
    lo = np.nanmin(kp.reshape(-1, 2), axis=0)
    kp = kp - lo
    W, H = (int(np.floor(e)) + 1 for e in np.nanmax(kp.reshape(-1, 2), axis=0))
    K = s["K"].copy()
    K[:, 0, 2] -= lo[0]
    K[:, 1, 2] -= lo[1]
    g = np.random.default_rng(seed)
    V, n = kp.shape[:2]
    seen = np.isfinite(kp).all(axis=2)
    m, c = np.zeros((len(ALL4), n, 4), f32), np.zeros((len(ALL4), n), f32)
    counts = np.zeros(len(ALL4), np.int32)
    for p, (a, b) in enumerate(ALL4):
        both = np.nonzero(seen[a] & seen[b])[0]
        k = len(both)
        xa = kp[a, both] + g.uniform(-jitter, jitter, (k, 2))
        xb = kp[b, both] + g.uniform(-jitter, jitter, (k, 2))
        m[p, :k] = np.stack([normalised(xa[:, 0], W), normalised(xa[:, 1], H), normalised(xb[:, 0], W), normalised(xb[:, 1], H)], axis=1)
        c[p, :k] = g.choice(np.array([1.0, 0.5, 0.2], f32), k)
        counts[p] = k
    case = dict(matches=m, certainty=c, counts=counts, pairs=ALL4, V=V, sizes=[(H, W)] * V)
    scene = dict(s, K=K, kpts=kp.astype(f32), seen2=int((seen.sum(axis=0) >= 2).sum()))
    return case, scene


def scene_tracks(o, case, K=16384):
    """tools/tracks_ref.py on a restated (or downloaded) result `o` of the operator"""
    return tkr.build(o["inds"], np.asarray(case["pairs"]), case["V"], K, case["counts"], o["num_kpts"], o["kpts"])


def chain_for(kp, K, rng_seed=3):
    """views_cases.ref_chain for arbitrary keypoints: kp [V, N, 2] float32 with NaN where a view does not observe the track,
    K [V, 3, 3].  Returns dict R, t, view_ok, or None without a seed pose."""
    kp = np.asarray(kp, f32)
    V = kp.shape[0]
    with np.errstate(invalid="ignore"):
        got = prr.estimate_pose(kp[0], kp[1], K[0], K[1], NORM_THR, conf=CONF, seed=rng_seed)
    if got is None:
        return None
    R, t = np.stack([np.eye(3)] * V), np.zeros((V, 3))
    R[1], t[1] = got[0], got[1].reshape(3)
    ok = np.zeros(V, dtype=bool)
    ok[:2] = True
    tri = tvr.triangulate(kp, K, R, t, view_valid=ok, max_reproj=THR)
    X = np.where((tri["flags"] == 0)[:, None], tri["points"], np.nan)
    for v in range(2, V):
        with np.errstate(invalid="ignore"):
            a = apr.estimate_absolute_pose(X.astype(f32).astype(np.float64), kp[v], K[v], THR, conf=CONF, seed=rng_seed + 1000003 * (v - 1))
        if a is not None:
            R[v], t[v], ok[v] = a[0], a[1].reshape(3), True
    tri = tvr.triangulate(kp, K, R, t, view_valid=ok, max_reproj=THR)
    X = np.where((tri["flags"] == 0)[:, None], tri["points"], np.nan)
    hold = br.default_hold(t) | ~ok[:, None]
    o = br.adjust(X, np.where(ok[:, None, None], kp, np.nan), K, R, t, THR, hold=hold)
    return dict(R=o["R"], t=o["t"], view_ok=ok)


def scene_pose_errors(scene, R, t, ok):
    """(rotation, translation direction) error in degrees against the scene, over the registered views"""
    return pose_errors(dict(R=scene["R"][ok], t=scene["t"][ok]), np.asarray(R)[ok], np.asarray(t)[ok])
