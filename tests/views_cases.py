"""What the multi-view tests share (test_cpu_views.py, test_gpu_views.py): the match graphs of the track builder, the scenes of
the N-view triangulation with the points whose trimming decisions rounding could turn, and the chain of numpy restatements
`reconstruct_views` is held against."""
import functools
import math
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import absolute_pose_ref as apr  # noqa: E402
import bundle_ref as br  # noqa: E402
import pose_refine_ref as prr  # noqa: E402
import tracks_ref as tkr  # noqa: E402
import triangulate_views_ref as tvr  # noqa: E402
from bundle_cases import pose_errors  # noqa: E402,F401
from bundle_scenes import scene  # noqa: E402

# ---- track builder: a case is a dict V, K, pairs [P, 2], inds [P, M, 2] (rows beyond match_counts hold rows that would change
# the result if they were read), match_counts [P], num_kpts [V] or None, x [V, K, 2] float32


def _pack(V, K, pairs, rows, num_kpts=None, junk=True, seed=0):
    """rows: one list of (i, j) per pair"""
    g = np.random.default_rng(seed)
    M = max(1, max(len(r) for r in rows)) + (2 if junk else 0)
    inds = g.integers(0, K, (len(pairs), M, 2)).astype(np.int32) if junk else np.full((len(pairs), M, 2), -1, dtype=np.int32)
    for p, r in enumerate(rows):
        if r:
            inds[p, :len(r)] = np.asarray(r, dtype=np.int32)
    x = (g.uniform(0, 640, (V, K, 2))).astype(np.float32)
    return dict(V=V, K=K, pairs=np.asarray(pairs, dtype=np.int32).reshape(-1, 2), inds=inds,
                match_counts=np.array([len(r) for r in rows], dtype=np.int32), num_kpts=None if num_kpts is None else np.asarray(num_kpts, dtype=np.int32), x=x)


def hand_made():
    """V = 3, K = 5: a consistent triangle on keypoints 0; a triangle that closes on another keypoint of view 0 (0:1 - 1:1 - 2:1 - 0:2),
    dropped; a duplicate row; a -1 row; an index >= num_kpts (view 1 has 4); the isolated keypoint 0:4; an empty pair; a pair given
    in the order (2, 1).  Expected: tracks (0, 0, 0) and (-1, 3, 3), info (8, 2, 3, 1)."""
    pairs = [(0, 1), (1, 2), (0, 2), (2, 1), (0, 2)]
    rows = [[(0, 0), (1, 1), (0, 0), (3, 4)], [(0, 0), (1, 1), (-1, -1)], [(0, 0), (2, 1)], [(3, 3)], []]
    return _pack(3, 5, pairs, rows, num_kpts=[5, 4, 5])


HAND_MADE_TRACKS = np.array([[0, -1], [0, 3], [0, 3]])
HAND_MADE_INFO = (8, 2, 3, 1)


def zigzag(permute, seed=3):
    """V = 2: one path a_0 - b_0 - a_1 - b_1 ... through 2 x 1025 keypoints, its rows shuffled - one component that holds both views
    1025 times, dropped - and ten separate 1-1 matches on the keypoints 1025 .. 1034 beside it, which come out as tracks.  (K is
    1035: a path through all of 2 x 1025 keypoints leaves none for the ten.)  permute: the path visits the keypoints of each view
    in a random order, so the labels do not fall along the path."""
    g = np.random.default_rng(seed)
    n, K = 1025, 1035
    a, b = (g.permutation(n), g.permutation(n)) if permute else (np.arange(n), np.arange(n))
    rows = [(a[i], b[i]) for i in range(n)] + [(a[i + 1], b[i]) for i in range(n - 1)] + [(n + i, n + 9 - i) for i in range(10)]
    rows = [rows[i] for i in g.permutation(len(rows))]
    return _pack(2, K, [(0, 1)], [rows], junk=False)


def planted(V, K, seed, n_tracks=None, false_frac=0.05, num_kpts=None, all_pairs=True):
    """planted tracks of 2 .. V views over the pairs of V views, each joined by a random connected set of its pairs' rows, plus
    false_frac rows between random keypoints (which merge tracks into components that hold a view twice)"""
    g = np.random.default_rng(seed)
    pairs = [(a, b) for a in range(V) for b in range(a + 1, V)]
    if not all_pairs:
        pairs = pairs[::2] + [pairs[0]]
    rows = {p: [] for p in range(len(pairs))}
    by_views = {}
    for p, (a, b) in enumerate(pairs):
        by_views.setdefault((a, b), []).append(p)
    nk = np.full(V, K) if num_kpts is None else np.asarray(num_kpts)
    free = [list(g.permutation(int(nk[v]))) for v in range(V)]
    for k in range(n_tracks if n_tracks is not None else (2 * K) // 3):
        L = 2 + k % (V - 1)
        views = sorted(g.choice(V, L, replace=False).tolist())
        if any(not free[v] for v in views):
            continue
        kp = {v: int(free[v].pop()) for v in views}
        order = list(g.permutation(L))
        edges = {tuple(sorted((views[order[i]], views[order[i + 1]]))) for i in range(L - 1)}  # a random path: connected
        edges |= {(views[i], views[j]) for i in range(L) for j in range(i + 1, L) if g.random() < 0.5}
        for a, b in edges:
            for p in by_views.get((a, b), []):
                rows[p].append((kp[a], kp[b]))
    for p, (a, b) in enumerate(pairs):
        for _ in range(int(false_frac * len(rows[p]))):
            rows[p].append((int(g.integers(0, K)), int(g.integers(0, K))))
        rows[p] = [rows[p][i] for i in g.permutation(len(rows[p]))]
    return _pack(V, K, pairs, [rows[p] for p in range(len(pairs))], num_kpts=num_kpts, seed=seed)


def track_ref(c, **kw):
    return tkr.build(c["inds"], c["pairs"], c["V"], c["K"], c["match_counts"], c["num_kpts"], c["x"], **kw)


# ---- N-view triangulation: the shapes of test_gpu_bundle.SHAPES
SHAPES = {"v2": (2, 65, 0.0, 0), "v3": (3, 513, 0.2, 1), "v8": (8, 130, 0.3, 2)}  # V, N, share of missing observations, seed
NOISY = dict(noise_px=0.5, outlier_frac=0.1)
THR = 2.0
EDGE = 1e-4  # a trimming decision whose worst error is within this (relative) of the threshold may fall either way


def f32(x):
    return np.asarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def tri_case(name, noisy, trim):
    """(scene with kpts as the device reads them, oracle result, points [N] bool left out of a comparison)"""
    V, n, miss, seed = SHAPES[name]
    s = scene(V, n, seed, missing=miss, **(NOISY if noisy else {}))
    s["kpts"] = f32(s["kpts"])
    trace = []
    o = tvr.triangulate(s["kpts"], s["K"], s["R"], s["t"], max_reproj=THR if noisy else math.inf, trim=trim, trace=trace)
    out = np.zeros(n, dtype=bool)
    for j, worst in trace:
        if abs(worst - 1.0) < EDGE:
            out[j] = True
    return s, o, out


# ---- reconstruct_views: the chain of the numpy restatements
NORM_THR = 1.0 / 520.0
CONF = 0.99999  # reconstruct_views' default, which it hands to both RANSAC runs


def views_scene(seed, noisy, dead_view=None):
    s = scene(4, 300, seed, missing=0.2, **(dict(noise_px=0.5, outlier_frac=0.05) if noisy else {}))
    s["kpts"] = f32(s["kpts"])
    if dead_view is not None:
        s["kpts"][dead_view] = np.nan
    return s


@functools.lru_cache(maxsize=None)
def ref_chain(seed, noisy, dead_view=None, rng_seed=3):
    """reconstruct_views from the numpy restatements (essential_ref / pose_refine_ref, triangulate_views_ref, absolute_pose_ref,
    bundle_ref) on views_scene: a dict R, t, points, view_ok, or None without a seed pose"""
    s = views_scene(seed, noisy, dead_view)
    kp, K = s["kpts"], s["K"]
    V, N = kp.shape[:2]
    with np.errstate(invalid="ignore"):  # the rows with a NaN stay in place, as on the device: never sampled, never inliers
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
        with np.errstate(invalid="ignore"):  # seeds as reconstruct_views derives them; the points as f32, as the device reads them
            a = apr.estimate_absolute_pose(X.astype(np.float32).astype(np.float64), kp[v], K[v], THR, conf=CONF, seed=rng_seed + 1000003 * (v - 1))
        if a is not None:
            R[v], t[v], ok[v] = a[0], a[1].reshape(3), True
    tri = tvr.triangulate(kp, K, R, t, view_valid=ok, max_reproj=THR)
    X = np.where((tri["flags"] == 0)[:, None], tri["points"], np.nan)
    hold = br.default_hold(t) | ~ok[:, None]
    o = br.adjust(X, np.where(ok[:, None, None], kp, np.nan), K, R, t, THR, hold=hold)
    return dict(R=o["R"], t=o["t"], points=o["points"], view_ok=ok, cost=(o["cost0"], o["cost"]), scene=s)


def chain_errors(seed, noisy, dead_view=None, rng_seed=3):
    """(rotation, translation direction) error in degrees of ref_chain against its scene, over the registered views"""
    r = ref_chain(seed, noisy, dead_view, rng_seed)
    s = r["scene"]
    ok = r["view_ok"]
    sub = dict(R=s["R"][ok], t=s["t"][ok])
    return pose_errors(sub, r["R"][ok], r["t"][ok])
