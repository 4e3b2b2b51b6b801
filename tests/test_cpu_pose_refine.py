"""tools/pose_refine_ref.py (the oracle of the device pose refinement, roma_amd.refine_pose) on the relief scene, and the C ABI
of roma_op_refine_pose (dlopen only).  No GPU."""
import glob
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_geometry import relief_scene

sys.path.insert(0, os.path.join(ROOT, "tools"))
import essential_ref as er  # noqa: E402
import pose_geometry as pg  # noqa: E402
import pose_refine_ref as pr  # noqa: E402

NEW_SYMBOLS = ("roma_op_refine_pose", "roma_op_refine_pose_workspace")
NOISY_CASES = [(noise, frac) for noise in (0.3, 1.0) for frac in (0.3, 0.5)]  # x RANSAC seeds 1 .. 6: the 24 cases
NOISY_SEEDS = (1, 2, 3, 4, 5, 6)


def pose_error(R, t, R0, t0):
    """max(e_R, e_t) in degrees against the pose (R0, t0); the sign of t is not observable"""
    e_t = pg.angle_error_vec(np.asarray(t).reshape(3), np.asarray(t0).reshape(3))
    return max(pg.angle_error_mat(R, R0), min(e_t, 180 - e_t))


def clean_scene(frac):
    """noise-free relief scene, 1 px threshold: (x0, x1 as the device reads them, thr, pose (R0, t0) of the scene's exact E, inlier
    truth)"""
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, noise_px=0, outlier_frac=frac)
    x0, x1 = pr.normalise(pa, pb, K, K)
    _, R0, t0, _ = pg.recover_pose(K.T @ F @ K, x0, x1, truth)
    return x0, x1, 1.0 / K[0, 0], R0, t0[:, 0], truth


def starts(R0, t0, degrees):
    """ten seeded starts `degrees` off in R and in t: one default_rng(0); per draw w then v = normal(3) scaled to the angle"""
    rng = np.random.default_rng(0)
    out = []
    for _ in range(10):
        w, v = rng.normal(size=3), rng.normal(size=3)
        w, v = w * np.deg2rad(degrees) / np.linalg.norm(w), v * np.deg2rad(degrees) / np.linalg.norm(v)
        out.append((pr.rodrigues(w) @ R0, pr.rodrigues(v) @ t0 / np.linalg.norm(t0)))
    return out


def noisy_case(noise, frac):
    """(K, T [3, 4] truth, pa, pb, thr) of one noise level and outlier rate of the issue's table"""
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, noise_px=noise, outlier_frac=frac)
    return K, np.c_[R, t], pa, pb, max(1.0, 2 * noise) / K[0, 0]


def test_jacobian_equals_central_differences():
    rng = np.random.default_rng(0)
    for _ in range(5):
        R = pr.rodrigues(rng.normal(size=3) * 0.3)
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        x0, x1 = rng.uniform(-0.5, 0.5, (200, 2)), rng.uniform(-0.5, 0.5, (200, 2))
        r, J = pr.jacobian(R, t, x0, x1)
        assert np.array_equal(r, pr.residuals(R, t, x0, x1))
        h = 1e-6
        Jn = np.zeros_like(J)
        for i in range(5):
            d = np.zeros(5)
            d[i] = h
            (Rp, tp), (Rm, tm) = pr.apply(R, t, d), pr.apply(R, t, -d)
            Jn[:, i] = (pr.residuals(Rp, tp, x0, x1) - pr.residuals(Rm, tm, x0, x1)) / (2 * h)
        assert np.abs(J - Jn).max() <= 1e-6 * np.abs(J).max(), np.abs(J - Jn).max() / np.abs(J).max()


def test_residual_is_the_sampson_distance_of_E():
    rng = np.random.default_rng(1)
    R, t = pr.rodrigues(rng.normal(size=3) * 0.2), np.array([0.6, -0.64, 0.48])
    x0, x1 = rng.uniform(-0.5, 0.5, (50, 2)), rng.uniform(-0.5, 0.5, (50, 2))
    r = pr.residuals(R, t, x0, x1)
    assert np.abs(r * r - pg.sampson_sq((pr.skew(t) @ R)[None], x0, x1)[0]).max() < 1e-15
    b = pr.tangent_basis(t)
    assert np.abs(b @ t).max() < 1e-15 and np.abs(b @ b.T - np.eye(2)).max() < 1e-15
    assert np.array_equal(b[0], np.cross(t, [0, 0, 1.0]) / np.linalg.norm(np.cross(t, [0, 0, 1.0])))  # |t_2| is the smallest


@pytest.mark.parametrize("frac", [0.0, 0.3, 0.5])
def test_exact_convergence_on_clean_data(frac):
    x0, x1, thr, R0, t0, truth = clean_scene(frac)
    for Rs, ts in starts(R0, t0, 0.01):
        o = pr.refine(Rs, ts, x0, x1, thr)
        # the bound of test_gpu_essential.test_exact_on_clean_data; measured 5e-6 (the resolution of arccos), 3 - 4 steps
        assert pose_error(o["R"], o["t"], R0, t0) < 1e-3 and 1 <= o["info"][0] <= 6 and o["info"][3] == 1
        # every inlier is active and in front of both cameras, no outlier is (they lie at least 2 px from the epipolar lines)
        assert o["cost"] <= o["cost0"] and np.array_equal(o["mask"], truth) and o["info"][2] == int(truth.sum())


def test_refinement_improves_the_noisy_cases():
    before, after = [], []
    for noise, frac in NOISY_CASES:
        K, T, pa, pb, thr = noisy_case(noise, frac)
        x0, x1 = pr.normalise(pa, pb, K, K)
        for seed in NOISY_SEEDS:
            R, t, mask = er.estimate_pose(pa, pb, K, K, thr, 0.99999, 1000, seed)
            o = pr.refine(R, t[:, 0], x0, x1, thr)
            assert o["cost"] <= o["cost0"] and o["info"][0] <= 25 and o["info"][1] <= 1 + 11 * 25
            assert np.array_equal(o["mask"], pr.active(pr.residuals(o["R"], o["t"], x0, x1), thr) &
                                  er.cheirality(o["R"], o["t"], x0, x1, 1e9))
            before.append(max(pg.compute_pose_error(T, R, t)))
            after.append(max(pg.compute_pose_error(T, o["R"], o["t"][:, None])))
    before, after = np.array(before), np.array(after)
    # measured with this oracle: lower in 23 of 24, median 1.56 -> 0.62 degrees, worst 3.72 -> 3.31
    assert (after < before).sum() >= 20 and np.median(after) < np.median(before), (before, after)


@pytest.mark.parametrize("frac,limit", [(0.0, 1), (0.3, 5)])
def test_degenerate_active_sets_return_the_input(frac, limit):
    """a start outside the threshold band: no active row (frac 0: nine of the ten starts) or fewer than the five parameters
    (frac 0.3: seven of ten) - H is singular, the input comes back with zero accepted steps"""
    x0, x1, thr, R0, t0, truth = clean_scene(frac)
    chosen = [(Rs, ts) for Rs, ts in starts(R0, t0, 1.0) if pr.cost(Rs, ts, x0, x1, thr)[1] < limit]
    assert len(chosen) >= 5
    for Rs, ts in chosen:
        o = pr.refine(Rs, ts, x0, x1, thr)
        assert np.array_equal(o["R"], Rs) and np.array_equal(o["t"], ts) and o["info"][0] == 0 and o["info"][3] == 1
        assert o["info"][1] == 1 and o["info"][2] == pr.cost(Rs, ts, x0, x1, thr)[1] and o["cost"] == o["cost0"]


def test_a_threshold_whose_square_is_not_finite_is_least_squares_over_the_finite_rows():
    """the loop's rule (lm_ref.truncated), which the pose shares with H and F: 1e200 is what the device call accepts, inf what
    only the oracle does; every finite row is active, the thr^2 (n - active) term is dropped, and `cost` is the same sum"""
    x0, x1, thr, R0, t0, truth = clean_scene(0.0)
    x0 = x0.copy()
    x0[[3, 700]] = np.nan
    Rs, ts = starts(R0, t0, 0.01)[0]
    fits = [pr.refine(Rs, ts, x0, x1, big) for big in (1e200, math.inf)]
    for o, big in zip(fits, (1e200, math.inf)):
        assert o["info"][0] >= 1 and o["info"][2:] == (len(x0) - 2, 1) and not o["mask"][[3, 700]].any()
        assert math.isfinite(o["cost"]) and o["cost"] < o["cost0"]
        assert pr.cost(o["R"], o["t"], x0, x1, big) == (o["cost"], len(x0) - 2)
        assert pose_error(o["R"], o["t"], R0, t0) < 1e-3
    assert np.array_equal(fits[0]["R"], fits[1]["R"]) and np.array_equal(fits[0]["t"], fits[1]["t"])


def test_invalid_pairs_and_the_solver_rule():
    x0, x1, thr, R0, t0, truth = clean_scene(0.0)
    for kw in (dict(valid=False), dict(max_steps=0)):
        o = pr.refine(R0, 2 * t0, x0, x1, thr, **kw)
        assert np.array_equal(o["R"], R0) and np.array_equal(o["t"], 2 * t0) and o["info"][0] == 0
    assert pr.refine(R0, t0, x0[:4], x1[:4], thr)["info"] == (0, 0, 0, 0)
    assert pr.refine(R0, np.zeros(3), x0, x1, thr)["info"][3] == 0
    H = np.diag([1.0, 2.0, 3.0, 4.0, 0.0])
    assert pr.solve(H, np.ones(5), 1e-3) is None                       # a zero pivot is not above 1e-14 x the largest diagonal
    H[4, 4] = 1e-3
    d = pr.solve(H, np.ones(5), 0.5)
    assert np.abs(d + 1 / (1.5 * np.diag(H))).max() < 1e-12


def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert built_lib.roma_op_refine_pose_workspace(8, 5000) > 0
    assert built_lib.roma_op_refine_pose_workspace(0, 10) == 0 and built_lib.roma_op_refine_pose_workspace(4, -1) == 0


def test_arguments_are_validated_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null address: validation must fail before it is used

    def call(*, R=p, t=p, a=p, out=p, B=1, N=10, thr=1e-3, steps=25, ws=p, nws=1 << 20):
        return lib.roma_op_refine_pose(R, t, a, p, None, None, B, N, thr, steps, out, p, p, p, ws, nws, None)
    for kw, word in ((dict(R=None), b"null"), (dict(t=None), b"null"), (dict(a=None), b"null"), (dict(out=None), b"null"),
                     (dict(ws=None), b"null"), (dict(B=0), b"B"), (dict(B=-1), b"B"), (dict(N=0), b"N"), (dict(N=-3), b"N"),
                     (dict(thr=0.0), b"threshold"), (dict(thr=-1.0), b"threshold"), (dict(thr=float("nan")), b"threshold"),
                     (dict(steps=-1), b"max_steps"), (dict(nws=16), b"workspace"), (dict(nws=-5), b"workspace")):
        assert call(**kw) != 0 and word in lib.roma_last_error(), kw


def test_refinement_refuses_host_tensors():
    import roma_amd
    from roma_amd import _lib
    x = torch.zeros(10, 2)
    K = torch.eye(3, dtype=torch.float64)
    calls = (lambda: roma_amd.refine_pose(torch.eye(3), torch.ones(3, 1), x, x, K, K, 1e-3),
             lambda: roma_amd.estimate_pose(x, x, K, K, 1e-3, refine=True),
             lambda: roma_amd.estimate_pose_uncalibrated(x, x, K, K, 1.0, refine=True))
    for call in calls:
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            call()


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_pose_refine_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "pose_refine.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/pose_refine.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    assert sorted(k["name"].split("::")[-1] for k in ks) == ["pose_refine_kernel", "pose_refine_mask_kernel"]
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
