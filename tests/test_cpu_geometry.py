"""tools/geometry_ref.py (the oracle of the device RANSAC, roma_amd.geometry) on exact synthetic geometry, its minimal solvers
and iteration formula, and the C ABI of roma_op_ransac (dlopen only).  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import geometry_ref as gr  # noqa: E402
import pose_geometry as pg  # noqa: E402
from accuracy_harness import synthetic_relief_pair  # noqa: E402


def _homography_scene(n=500, outlier_frac=0.4, thr=3.0, seed=0, size=864):
    rng = np.random.default_rng(seed)
    H = np.array([[1.08, 0.06, 25.0], [-0.04, 0.93, 14.0], [1.2e-4, -6e-5, 1.0]])
    pa = rng.uniform(0, size, (n, 2))
    ph = np.c_[pa, np.ones(n)] @ H.T
    pb = ph[:, :2] / ph[:, 2:]
    out = rng.random(n) < outlier_frac
    pb[out] += rng.uniform(10 * thr, 30 * thr, (out.sum(), 2)) * rng.choice([-1.0, 1.0], (out.sum(), 2))
    return H, pa, pb, ~out


def relief_scene(h=480, w=640, seed=3, n=600, outlier_frac=0.3, thr=0.2, rng_seed=1, noise_px=0.0):
    """The relief scene of accuracy_harness.synthetic_relief_pair with exact f64 correspondences: each visible grid point's depth
    is triangulated from the pair's (f32) match and re-projected, so every inlier lies on the true epipolar geometry to f64
    rounding (plus noise_px of Gaussian noise in image B).  Outliers sit at least 10 thr from both epipolar lines of the true F.  Returns (K, R, t, F, pa, pb, inlier truth).
    The relief is close to a plane at this baseline: for some scene seeds a wrong epipolar geometry through all the inliers
    and one or two outliers out-counts the true one, which is RANSAC's correct answer to that data - seed 3 has none."""
    d = synthetic_relief_pair(h, w, seed=seed)
    K, T = d["K1"], d["T_1to2"]
    R, t = T[:, :3], T[:, 3]
    m = d["gt_matches"].double().numpy().reshape(-1, 4)
    vis = d["gt_certainty"].numpy().reshape(-1) > 0
    rng = np.random.default_rng(rng_seed)
    sel = rng.choice(np.nonzero(vis)[0], n, replace=False)
    pa = np.stack([(m[sel, 0] + 1) * w / 2, (m[sel, 1] + 1) * h / 2], 1)
    p2 = np.stack([(m[sel, 2] + 1) * w / 2, (m[sel, 3] + 1) * h / 2], 1)
    ray = np.c_[pa, np.ones(n)] @ np.linalg.inv(K).T
    Kr, Kt = ray @ (K @ R).T, K @ t
    # p2 (Kr z + Kt)_2 = (Kr z + Kt)_{0,1}: least squares in z over both coordinates
    ax, bx = Kr[:, 0] - p2[:, 0] * Kr[:, 2], p2[:, 0] * Kt[2] - Kt[0]
    ay, by = Kr[:, 1] - p2[:, 1] * Kr[:, 2], p2[:, 1] * Kt[2] - Kt[1]
    z = (ax * bx + ay * by) / (ax * ax + ay * ay)
    q = Kr * z[:, None] + Kt
    pb = q[:, :2] / q[:, 2:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    pb = pb + noise_px * rng.normal(size=pb.shape)
    out = rng.random(n) < outlier_frac
    for i in np.nonzero(out)[0]:
        while True:
            c = rng.uniform([0, 0], [w, h])
            if min(epipolar_dist(F, pa[i:i + 1], c[None])) > 10 * thr:
                pb[i] = c
                break
    return K, R, t, F, pa, pb, ~out


def epipolar_dist(F, pa, pb):
    """(distance of x_B to F x_A in image B, distance of x_A to F^T x_B in image A), pixels"""
    ha, hb = np.c_[pa, np.ones(len(pa))], np.c_[pb, np.ones(len(pb))]
    la, lb = ha @ F.T, hb @ F
    d = np.abs((hb * la).sum(1))
    return d / np.hypot(la[:, 0], la[:, 1]), d / np.hypot(lb[:, 0], lb[:, 1])


@pytest.mark.parametrize("refine", [False, True])
def test_reference_homography_exact_on_noise_free_scene(refine):
    H, pa, pb, truth = _homography_scene()
    r = gr.ransac(gr.HOMOGRAPHY, pa, pb, 3.0, 0.995, 2000, seed=7, refine=refine)
    assert r["ok"]
    assert np.abs(r["M"] - H).max() / np.abs(H).max() < 1e-9
    assert np.array_equal(r["mask"], truth)
    Hr, mask = gr.find_homography(pa, pb, 3.0, seed=7)
    assert np.array_equal(mask, truth) and abs(Hr[2, 2] - 1) < 1e-15


@pytest.mark.parametrize("refine", [False, True])
def test_reference_fundamental_exact_on_relief_scene_and_pose(refine):
    K, R, t, Ft, pa, pb, truth = relief_scene()
    F, mask = gr.find_fundamental(pa, pb, 0.2, 0.999, 2000, seed=11, refine=refine)
    assert F is not None and np.array_equal(mask, truth)
    assert abs(np.linalg.det(F)) < 1e-12 * np.linalg.norm(F) ** 3 and abs(F[2, 2] - 1) < 1e-15
    da, db = epipolar_dist(F, pa[truth], pb[truth])
    # the refit on all 400+ inliers is exact to f64 rounding; a minimal 7-point sample of a near-planar scene loses a few digits
    assert max(da.max(), db.max()) < (1e-9 if refine else 1e-7), (da.max(), db.max())
    E = K.T @ F @ K
    Ki = np.linalg.inv(K)
    x0, x1 = (np.c_[pa, np.ones(len(pa))] @ Ki.T)[:, :2], (np.c_[pb, np.ones(len(pb))] @ Ki.T)[:, :2]
    n, Rp, tp, _ = pg.recover_pose(E, x0, x1, mask)
    assert n > 0.9 * truth.sum()
    # angles from chord / cross-product norms: arccos of the trace cannot resolve 1e-6 rad, and the scene's R is orthonormal to
    # ~3e-8 only (synthetic_relief_pair forms it from f32 sines)
    e_R = np.linalg.norm(Rp - R) / math.sqrt(2)
    tu, tv = tp[:, 0] / np.linalg.norm(tp), t / np.linalg.norm(t)
    e_t = np.linalg.norm(np.cross(tu, tv))
    assert e_R < 1e-6 and e_t < 1e-6, (e_R, e_t)


def test_seven_point_solver_models_satisfy_the_sample_and_are_singular():
    rng = np.random.default_rng(5)
    xa, xb = rng.normal(size=(200, 7, 2)), rng.normal(size=(200, 7, 2))
    F, n = gr.solve_f(xa, xb)
    assert set(np.unique(n)) <= {1, 3} and (n == 1).any() and (n == 3).any()
    for i in range(len(xa)):
        for k in range(n[i]):
            f = F[i, k]
            res = np.einsum("ni,ij,nj->n", np.c_[xb[i], np.ones(7)], f, np.c_[xa[i], np.ones(7)])
            assert np.abs(res).max() < 1e-10 and abs(np.linalg.det(f)) < 1e-10
            assert abs(np.linalg.norm(f) - 1) < 1e-12
    # a degenerate sample (all points on one line in both images) yields no model
    s = np.linspace(-1, 1, 7)
    line = np.stack([s, 0.5 * s + 0.1], 1)[None]
    assert gr.solve_f(line, 2 * line)[1][0] == 0


def test_dlt_rejects_collinear_and_orientation_flipped_samples():
    xa = np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]])
    H = np.array([[1.1, 0.1, 0.2], [0.05, 0.9, -0.1], [0.02, 0.01, 1.0]])
    ph = np.c_[xa[0], np.ones(4)] @ H.T
    xb = (ph[:, :2] / ph[:, 2:])[None]
    Hs, ok = gr.solve_h(xa, xb)
    assert ok[0] and np.abs(Hs[0] / Hs[0, 2, 2] - H / H[2, 2]).max() < 1e-12
    col = xa.copy()
    col[0, 2] = [0.5, 0.0]  # three points on y = 0
    assert not gr.solve_h(col, xb)[1][0] and not gr.solve_h(xb, col)[1][0]
    flip = xb.copy()
    flip[0, [2, 3]] = flip[0, [3, 2]]  # two triples keep their orientation, two flip
    assert not gr.h_subset_ok(xa, flip)[0] and not gr.solve_h(xa, flip)[1][0]
    mirror = xb * np.array([-1.0, 1.0])  # a reflection flips all four triples: OpenCV keeps it
    assert gr.h_subset_ok(xa, mirror)[0]


@pytest.mark.parametrize("w,conf,s", [(0.5, 0.995, 4), (0.7, 0.999999, 7), (0.3, 0.99, 7), (0.9, 0.995, 4)])
def test_adaptive_iteration_count_matches_direct_evaluation(w, conf, s):
    want = math.ceil(math.log(1 - conf) / math.log(1 - w ** s))
    assert gr.update_num_iters(conf, w, s, 10 ** 9) == want
    assert gr.update_num_iters(conf, w, s, 10) == min(10, want)
    assert gr.update_num_iters(conf, 1.0, s, 1000) == 0  # every point an inlier: nothing more to draw
    assert gr.update_num_iters(conf, 0.0, s, 1000) == 1000


def test_sampling_stream_depends_only_on_seed_and_hypothesis():
    a, ok = gr.draw_samples(99, np.arange(0, 512), 50, 7)
    b, _ = gr.draw_samples(99, np.arange(256, 512), 50, 7)
    assert ok.all() and np.array_equal(a[256:], b)
    assert all(len(set(row)) == 7 for row in a) and a.min() >= 0 and a.max() < 50
    assert not np.array_equal(gr.draw_samples(100, np.arange(256), 50, 7)[0], a[:256])
    # exactly the minimal number of rows: the redraw counter still finds a permutation for most hypotheses
    idx, ok = gr.draw_samples(3, np.arange(256), 4, 4)
    assert ok.mean() > 0.99 and all(sorted(r) == [0, 1, 2, 3] for r in idx[ok])


def test_ransac_is_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in ("roma_op_ransac", "roma_op_ransac_workspace"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert built_lib.roma_op_ransac_workspace(8, 10000) > 8 * 10000 * 16
    # argument validation happens before any device work
    rc = built_lib.roma_op_ransac(2, None, None, None, None, 1, 10, 1.0, 0.99, 100, 1, None, None, None, None, None, 0, None)
    assert rc != 0 and b"model" in built_lib.roma_last_error()


def test_find_functions_refuse_host_tensors():
    import roma_amd
    from roma_amd import _lib
    x = torch.zeros(10, 2)
    for fn in (roma_amd.find_homography, roma_amd.find_fundamental):
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            fn(x, x)
