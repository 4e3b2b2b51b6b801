"""tools/essential_magsac_ref.py (the oracle of the device MAGSAC++ scoring and local optimisation of essential-matrix RANSAC,
roma_amd.geometry.essential_magsac): its residual, exact fits on noise-free scenes, its accuracy against plain five-point RANSAC
(tools/essential_ref.py) on the noisy relief scenes, the C ABI of roma_op_essential_magsac (dlopen only) and the resources of
its kernels.  No GPU."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_geometry import relief_scene
from test_cpu_pose_refine import NOISY_CASES, NOISY_SEEDS, noisy_case, pose_error

sys.path.insert(0, os.path.join(ROOT, "tools"))
import essential_magsac_ref as em  # noqa: E402
import essential_ref as er  # noqa: E402
import pose_geometry as pg  # noqa: E402
import pose_refine_ref as pr  # noqa: E402

NEW_SYMBOLS = ("roma_op_essential_magsac", "roma_op_essential_magsac_workspace")
# test_oracle_beats_five_point_ransac_on_the_noisy_cases: medians of max(e_R, e_t) in degrees over the 24 cases, (five-point RANSAC,
# MAGSAC++ with LO); tests/test_gpu_essential_magsac.py holds the device to their ratio
ORACLE_MEDIANS = (1.562648, 0.133890)
ORACLE_RATIO = ORACLE_MEDIANS[1] / ORACLE_MEDIANS[0]  # 0.08568


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert built_lib.roma_op_essential_magsac_workspace(8, 5000) >= built_lib.roma_op_essential_workspace(8, 5000)
    assert built_lib.roma_op_essential_magsac_workspace(0, 10) == 0 and built_lib.roma_op_essential_magsac_workspace(4, -1) == 0


def test_arguments_are_validated_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null address: validation must fail before it is used

    def call(*, a=p, seeds=p, e=p, score=p, B=1, N=10, thr=1.0, prob=0.99, iters=100, lo=10, ws=p, nws=1 << 30):
        return lib.roma_op_essential_magsac(a, p, None, seeds, None, B, N, thr, prob, iters, lo, e, p, p, p, score, ws, nws, None)
    for kw, word in ((dict(a=None), b"null"), (dict(seeds=None), b"null"), (dict(e=None), b"null"), (dict(score=None), b"null"),
                     (dict(ws=None), b"null"), (dict(B=0), b"B"), (dict(B=-1), b"B"), (dict(N=0), b"N"), (dict(N=-3), b"N"),
                     (dict(thr=0.0), b"threshold"), (dict(thr=float("nan")), b"threshold"), (dict(prob=1.5), b"prob"),
                     (dict(iters=0), b"max_iters"), (dict(lo=-1), b"lo_iters"), (dict(lo=65), b"lo_iters"),
                     (dict(nws=16), b"workspace"), (dict(nws=-5), b"workspace")):
        assert call(**kw) != 0 and word in lib.roma_last_error(), kw
        assert b"essential_magsac" in lib.roma_last_error()
    # roma_op_magsac still takes the homography and the fundamental matrix only
    assert lib.roma_op_magsac(2, p, p, None, p, 1, 10, 1.0, 0.99, 100, 10, p, p, p, p, p, p, 1 << 30, None) != 0
    assert b"model" in lib.roma_last_error()


def test_new_functions_refuse_host_tensors_and_unknown_methods():
    import roma_amd
    from roma_amd import _lib
    x = torch.zeros(10, 2)
    K = torch.eye(3, dtype=torch.float64)
    calls = (lambda: roma_amd.essential_magsac(x, x), lambda: roma_amd.find_essential(x, x, method="magsac"),
             lambda: roma_amd.estimate_pose(x, x, K, K, 1e-3, method="magsac"),
             lambda: roma_amd.estimate_pose(x, x, K, K, 1e-3, method="magsac", refine=True),
             lambda: roma_amd.estimate_pose_uncalibrated(x, x, K, K, 1.0, method="magsac"))
    for call in calls:
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            call()
    for call in (lambda: roma_amd.find_essential(x, x, method="lmeds"), lambda: roma_amd.estimate_pose(x, x, K, K, 1e-3, method="lmeds"),
                 lambda: roma_amd.estimate_pose_uncalibrated(x, x, K, K, 1.0, method="usac")):
        with pytest.raises(ValueError, match="method must be 'ransac' or 'magsac'"):
            call()


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_residual_is_the_sampson_distance():
    rng = np.random.default_rng(0)
    E = rng.normal(size=(6, 3, 3))
    x0, x1 = rng.uniform(-0.6, 0.6, (300, 2)), rng.uniform(-0.6, 0.6, (300, 2))
    r2, s2 = em.residual2(E, x0, x1), pg.sampson_sq(E, x0, x1)
    # d = x1^T E x0 is a sum of nine products: where it cancels to less than 1 % of their magnitudes either formula is further
    # than 1e-12 from the exact value (2^-53 x 100 x a few operations, squared residual), so those rows cannot tell them apart
    h0, h1 = np.c_[x0, np.ones(len(x0))], np.c_[x1, np.ones(len(x1))]
    mag = np.einsum("ni,kij,nj->kn", np.abs(h1), np.abs(E), np.abs(h0))
    d = np.einsum("ni,kij,nj->kn", h1, E, h0)
    well = np.abs(d) >= 0.01 * mag
    assert well.mean() > 0.95
    assert np.abs(r2 / s2 - 1)[well].max() < 1e-12
    assert np.abs(r2 - s2).max() < 1e-12 * s2.max()
    r32 = em.residual2(E, x0, x1, f32=True)
    assert np.abs(r32 / s2 - 1).max() < 1e-3 and (r32 != r2).any()
    # V = r^2 k^2 / (2 tau^2) in the units of the residual: tau is the camera-normalised threshold
    K = np.array([[500.0, 0, 320], [0, 520.0, 240], [0, 0, 1]])
    pa, pb = x0 * [500, 520] + [320, 240], x1 * [500, 520] + [320, 240]
    S, rho, w, V = em.scores(pa, pb, 2.0, E, K=K)
    assert np.abs(V / (s2 * em.mr.K2 / (2 * (2.0 / 510.0) ** 2)) - 1).max() < 1e-9


def test_oracle_exact_on_clean_data():
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, outlier_frac=0.3)
    x0, x1 = pr.normalise(pa, pb, K, K)
    r = em.magsac(x0, x1, 0.5 / K[0, 0], 0.999, 1000, seed=1)
    assert r["ok"] and np.array_equal(r["mask"], truth) and r["score"] <= r["score_min"] and r["lo_steps"] <= em.LO_ITERS
    E = r["E"]
    s = np.linalg.svd(E, compute_uv=False)
    assert abs(s[0] - s[1]) < 1e-12 and s[2] < 1e-12 and abs(np.linalg.norm(E) - 1) < 1e-12 and E.flat[np.argmax(np.abs(E))] > 0
    _, R0, t0, _ = pg.recover_pose(K.T @ F @ K, x0, x1, truth)
    _, Rp, tp, good = er.recover_pose(E, x0, x1, r["mask"])
    # the bound of tests/test_gpu_essential.py::test_exact_on_clean_data
    assert pose_error(Rp, tp, R0, t0) < 1e-3, pose_error(Rp, tp, R0, t0)
    assert np.array_equal(good, truth)


def test_oracle_without_lo_keeps_the_minimal_model():
    K, T, pa, pb, thr = noisy_case(0.3, 0.3)
    x0, x1 = pr.normalise(pa, pb, K, K)
    r = em.magsac(x0, x1, thr, 0.99999, 1000, seed=2, lo_iters=0)
    assert r["ok"] and r["lo_steps"] == 0 and r["score"] == r["score_min"] and r["best"] == r["best_min"]
    m = em.minimal_model(x0, x1, 2, r["best_h"], r["best_root"])
    assert np.array_equal(r["E"], m)
    assert em.scores(x0, x1, thr, m[None])[0][0] == r["score_min"]
    assert np.array_equal(r["mask"], er.inliers(m[None], x0, x1, thr * thr)[0])  # find_essential's inlier rule
    assert em.minimal_model(x0, x1, 2, r["best_h"], 10) is None


def test_oracle_refit_needs_eight_weighted_rows_and_lands_on_the_manifold():
    K, T, pa, pb, thr = noisy_case(0.3, 0.0)
    x0, x1 = pr.normalise(pa, pb, K, K)
    w = np.zeros(len(x0))
    w[:7] = 1.0
    assert em.weighted_refit(x0, x1, w, lambda Es: np.zeros(len(Es))) is None
    w[:40] = 1.0
    basis = em.refit_basis(x0, x1, w)
    assert np.abs(basis.T @ basis - np.eye(4)).max() < 1e-12
    E = em.weighted_refit(x0, x1, w, lambda Es: em.residual2(Es, x0[:40], x1[:40]).sum(axis=1))
    s = np.linalg.svd(E, compute_uv=False)
    assert abs(s[0] - s[1]) < 1e-12 and s[2] < 1e-12 and abs(np.linalg.norm(E) - 1) < 1e-12 and E.flat[np.argmax(np.abs(E))] > 0
    assert np.sqrt(em.residual2(E[None], x0[:40], x1[:40])[0]).mean() < thr  # 0.3 px of noise, threshold 1 px


def test_oracle_beats_five_point_ransac_on_the_noisy_cases():
    """max(e_R, e_t) in degrees over the 24 noisy cases, essential_ref.estimate_pose (five-point RANSAC, the winning sample as it
    is) vs essential_magsac_ref.estimate_pose with the same seed and threshold: median 1.5626 -> 0.1339, ratio 0.0857, lower in
    24 of 24 (worst case 3.72 -> 0.57).  MAGSAC++ scoring alone (lo_iters = 0) gives a median of 1.4264.  With the candidate of
    the plain eight-point algorithm (the smallest eigenvector projected onto the essential manifold) as the LO step, the
    candidate lowered the score in 4 of the 24 cases and the median stayed at 1.5626: the relief is close to a plane, where that
    eigenvector follows the noise (essential_magsac_ref.weighted_refit)."""
    a, b = [], []
    for noise, frac in NOISY_CASES:
        K, T, pa, pb, thr = noisy_case(noise, frac)
        for seed in NOISY_SEEDS:
            R, t, _ = er.estimate_pose(pa, pb, K, K, thr, 0.99999, 1000, seed)
            a.append(max(pg.compute_pose_error(T, R, t)))
            R, t, _ = em.estimate_pose(pa, pb, K, K, thr, 0.99999, 1000, seed)
            b.append(max(pg.compute_pose_error(T, R, t)))
    a, b = np.array(a), np.array(b)
    ma, mb = float(np.median(a)), float(np.median(b))
    print(f"five-point RANSAC {np.round(a, 3)}\nMAGSAC++ {np.round(b, 3)}\nmedians {ma:.4f} -> {mb:.4f}, ratio {mb / ma:.4f}, "
          f"lower in {(b < a).sum()} of {len(a)}")
    assert mb < ma
    # the figures the GPU tests compare the device with
    assert abs(ma / ORACLE_MEDIANS[0] - 1) < 0.01 and abs(mb / ORACLE_MEDIANS[1] - 1) < 0.05, (ma, mb)


# ---------------------------------------------------------------------------------------------------------------- resources
@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_essential_magsac_kernels_have_no_spills_and_no_scratch(build):
    """the ten-slot score kernel and the refit (9 x 9 eigenproblem, five-point solver, ten-slot scoring) live in registers and LDS"""
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "essential.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/essential.o not built")
    import kernel_resources
    ks = [k for k in kernel_resources.kernels(obj) if "Essential" in k["name"]]
    names = sorted(re.sub(r"(roma::)?\(anonymous namespace\)::", "", k["name"]) for k in ks)
    # every kernel of the shared pipeline (ransac.h) instantiated on Essential, under both scorings
    assert names == ["magsac_init_kernel<Essential>", "ransac_accept_kernel<Essential, MagsacScoring>",
                     "ransac_finish_kernel<Essential, CountScoring>", "ransac_finish_kernel<Essential, MagsacScoring>",
                     "ransac_hyp_kernel<Essential>", "ransac_mask_kernel<Essential, CountScoring>",
                     "ransac_mask_kernel<Essential, MagsacScoring>", "ransac_norm_kernel<Essential>",
                     "ransac_refit_kernel<Essential, MagsacScoring>", "ransac_score_kernel<Essential, CountScoring>",
                     "ransac_score_kernel<Essential, MagsacScoring>", "ransac_select_kernel<Essential, CountScoring>",
                     "ransac_select_kernel<Essential, MagsacScoring>"], names
    for k in ks:
        assert "Essential" in k["name"]
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert k["lds"] <= 64 * 1024, k
