"""The scenes shared by tests/test_cpu_gt_warp.py and tests/test_gpu_gt_warp.py (and recorded, with the reference's outputs on them,
in tests/golden/gt_warp_reference.npz by tools/make_gt_warp_goldens.py).  The smallest scene that takes every branch of warp_kpts:

  pairs 0-2  a tilted plane at distance ~2 seen by two different cameras (principal points off centre, fx != fy; roll +-0.06 rad, yaw
             +-0.12 rad, translation up to (0.17, 0.1, -0.15)); depth0 23 x 31, depth1 19 x 37; a 4 x 5 block of zeros in depth0 (zero
             depth inside, blended non-zero-but-wrong depth on its rim), a 5 x 7 block of depth1 scaled by 0.8 (inconsistent rows), a
             3 x 5 block of zeros in depth1 (division by zero: rel = inf);
  pair 3     the same with t_z = 0, t_x != 0: the rows of the zero block of depth0 project through the bare 1e-4, land tens of
             thousands of pixels outside, sample 0 and give rel = |0 / 0| = NaN.

Key points: the 17 x 29 grid plus 510 uniform in [-1.2, 1.2]^2 (some outside image 0), L = 1003 = 3 workgroups + 235 rows, all
float32 values so that the float32 and the float64 form hold the same numbers.  Metric input: a 17 x 29 warp whose B half is the
oracle's warp of the grid plus N(0, 0.08) noise - the pixel scale (17, 29) is neither depth map's size."""
import functools
import os
import sys

import numpy as np

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gt_warp_ref as gw  # noqa: E402

B = 4
H0, W0, H1, W1 = 23, 31, 19, 37
GRID_H, GRID_W = 17, 29
N_RANDOM = 510
L = GRID_H * GRID_W + N_RANDOM
THRESHOLD = 0.05
PCK = (1.0, 3.0, 5.0)
NOISE = 0.08


def _rot(roll, yaw):
    cz, sz, cy, sy = np.cos(roll), np.sin(roll), np.cos(yaw), np.sin(yaw)
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    return Ry @ Rz


def _plane_depth(K, H, W, nrm, dist):
    """depth of the plane nrm . X = dist along the rays of the pixel centres"""
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    rays = np.stack([xs, ys, np.ones_like(xs)], axis=-1) @ np.linalg.inv(K).T
    return dist / (rays @ nrm)


def _pair(seed, flat_tz=False):
    rng = np.random.default_rng(seed)
    s = lambda: 2.0 * rng.random() - 1.0  # noqa: E731
    K0 = np.array([[27.0 + 2.0 * rng.random(), 0.0, W0 / 2 + 1.3 * s()], [0.0, 24.0 + 2.0 * rng.random(), H0 / 2 + 1.1 * s()], [0.0, 0.0, 1.0]])
    K1 = np.array([[31.0 + 2.0 * rng.random(), 0.0, W1 / 2 + 1.3 * s()], [0.0, 22.0 + 2.0 * rng.random(), H1 / 2 + 1.1 * s()], [0.0, 0.0, 1.0]])
    R = _rot(0.06 * s(), 0.12 * s())
    t = np.array([0.17 * s(), 0.1 * s(), -0.15 * rng.random()])
    if flat_tz:
        t[0], t[2] = 0.11, 0.0
    nrm = np.array([0.2 * s(), 0.15 * s(), 1.0])
    nrm = nrm / np.linalg.norm(nrm)
    dist = 2.0
    depth0 = _plane_depth(K0, H0, W0, nrm, dist)
    n1 = R @ nrm
    depth1 = _plane_depth(K1, H1, W1, n1, dist + n1 @ t)
    depth0[8:12, 11:16] = 0.0
    depth1[3:8, 20:27] *= 0.8
    depth1[11:14, 6:11] = 0.0
    T = np.concatenate([R, t[:, None]], axis=1)
    kp = np.concatenate([gw.grid(GRID_H, GRID_W), rng.uniform(-1.2, 1.2, (N_RANDOM, 2)).astype(np.float32)], axis=0)
    return {"kpts": kp.astype(np.float32), "depth0": depth0.astype(np.float32), "depth1": depth1.astype(np.float32), "T": T, "K0": K0, "K1": K1}


INPUTS = ("kpts", "depth0", "depth1", "T", "K0", "K1", "matches")
GOLDEN_FILE = os.path.join(GOLDEN, "gt_warp_reference.npz")


def build_scene():
    """the scene from its seeds - what tools/make_gt_warp_goldens.py records.  dict of arrays with the batch axis: kpts f32 [B, L, 2],
    depth0 f32 [B, H0, W0], depth1 f32 [B, H1, W1], T f64 [B, 3, 4], K0, K1 f64 [B, 3, 3], matches f32 [B, GRID_H, GRID_W, 4]"""
    pairs = [_pair(0), _pair(1), _pair(2), _pair(3, flat_tz=True)]
    out = {k: np.stack([p[k] for p in pairs]) for k in pairs[0]}
    rng = np.random.default_rng(100)
    grid = gw.grid(GRID_H, GRID_W)
    matches = np.empty((B, GRID_H, GRID_W, 4), dtype=np.float32)
    for b in range(B):
        x2 = gw.warp_kpts(grid, out["depth0"][b], out["depth1"][b], out["T"][b], out["K0"][b], out["K1"][b], THRESHOLD)["warped"]
        x2 = x2 + NOISE * rng.standard_normal(x2.shape)
        matches[b] = np.concatenate([grid, x2.astype(np.float32)], axis=-1).reshape(GRID_H, GRID_W, 4)
    out["matches"] = matches
    return out


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/gt_warp_reference.npz: the scene (in_*) and what the unmodified reference returned on it (ref_*)"""
    with np.load(GOLDEN_FILE) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene():
    """the recorded scene (the bits the reference ran on, whatever this machine's libm makes of build_scene): read-only arrays"""
    g = golden()
    return {k: g["in_" + k] for k in INPUTS}


@functools.lru_cache(maxsize=None)
def oracle():
    """what tools/gt_warp_ref.py makes of the scene, computed once: per pair lists `warp` (warp_kpts on the key points), `gt` (get_gt_warp
    at depth0's size), `gt_grid` (get_gt_warp on the GRID_H x GRID_W grid) and `metrics` (dense_metrics)"""
    s = scene()
    out = {"warp": [], "gt": [], "gt_grid": [], "metrics": []}
    for b in range(B):
        a = (s["depth0"][b], s["depth1"][b], s["T"][b], s["K0"][b], s["K1"][b], THRESHOLD)
        out["warp"].append(gw.warp_kpts(s["kpts"][b], *a))
        out["gt"].append(gw.get_gt_warp(*a))
        out["gt_grid"].append(gw.get_gt_warp(*a, H=GRID_H, W=GRID_W))
        out["metrics"].append(gw.dense_metrics(s["matches"][b], *a, thresholds=PCK))
    return out


def batch_means(metrics):
    """(epe, pck [3], n, gd_sum) over all valid pixels of a list of per-pair dense_metrics dicts, the pairs in order"""
    n = sum(m["n_valid"] for m in metrics)
    total = 0.0
    for m in metrics:
        total = total + m["gd_sum"]
    below = np.sum([m["n_below"] for m in metrics], axis=0)
    with np.errstate(all="ignore"):
        return np.float64(total) / np.float64(n), below.astype(np.float64) / np.float64(n), n, total
