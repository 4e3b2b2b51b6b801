"""tools/model_refine_ref.py (the oracle of the device refinement of homographies and fundamental matrices,
roma_amd.refine_homography / refine_fundamental) on the synthetic scenes, and the C ABI of roma_op_refine_model (dlopen only).
No GPU."""
import functools
import glob
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_geometry import _homography_scene, epipolar_dist, relief_scene

sys.path.insert(0, os.path.join(ROOT, "tools"))
import geometry_ref as gr  # noqa: E402
import model_refine_ref as mr  # noqa: E402

H, F = mr.HOMOGRAPHY, mr.FUNDAMENTAL
NEW_SYMBOLS = ("roma_op_refine_model", "roma_op_refine_model_workspace")
FRACS = (0.0, 0.3, 0.5)
NOISY_CASES = [(noise, frac) for noise in (0.3, 1.0) for frac in (0.3, 0.5)]  # x RANSAC seeds 1 .. 6: 24 cases per model
NOISY_SEEDS = (1, 2, 3, 4, 5, 6)
CLEAN_THR = {H: 3.0, F: 1.0}  # px: the H scene's outliers lie 30 px and more away, the relief's 2 px and more from both lines
SIZE = 864  # the frame of _homography_scene
MAX_STEPS = 25


def corner_error(M, M0, size=SIZE):
    """the HPatches measure: mean distance of the frame's four corners mapped by M and by M0, pixels"""
    c = np.array([[0, 0, 1], [size, 0, 1], [size, size, 1], [0, size, 1.0]])
    a, b = c @ np.asarray(M).T, c @ np.asarray(M0).T
    return float(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1).mean())


def epipolar_error(M, pa, pb, reduce=np.mean):
    """epipolar distance (both images) of the noise-free inliers pa, pb under M, pixels"""
    da, db = epipolar_dist(np.asarray(M), pa, pb)
    return float(reduce(np.r_[da, db]))


@functools.lru_cache(maxsize=None)
def scene(model, frac, noise=0.0):
    """(true model scaled to [2, 2] = 1, pa, pb, inlier truth, noise-free pa, pb of the inliers) with n = 2 000; the noise of
    the homography scene, which has none of its own, is Gaussian in image B from default_rng(100)"""
    if model == H:
        M, pa, pb, truth = _homography_scene(n=2000, outlier_frac=frac)
        clean = (pa[truth], pb[truth].copy())
        if noise:
            pb = pb + noise * np.random.default_rng(100).normal(size=pb.shape)
        return M, pa, pb, truth, clean
    _, _, _, M, pa, pb, truth = relief_scene(n=2000, noise_px=noise, outlier_frac=frac)
    _, _, _, _, pa0, pb0, truth0 = relief_scene(n=2000, noise_px=0, outlier_frac=frac)
    assert np.array_equal(pa, pa0) and np.array_equal(truth, truth0)
    return M / M[2, 2], pa, pb, truth, (pa0[truth], pb0[truth])


def error(model, M, frac, noise=0.0):
    """the error of M against the scene's truth: mean corner error (H), mean epipolar distance of the noise-free inliers (F)"""
    M0, _, _, _, clean = scene(model, frac, noise)
    return corner_error(M, M0) if model == H else epipolar_error(M, *clean)


def starts(model, M0):
    """ten seeded starts around the true model: every entry scaled by 1 + 1e-4 normal, one default_rng(0) (for F the start is
    then of full rank, which the fit projects)"""
    rng = np.random.default_rng(0)
    return [M0 * (1 + 1e-4 * rng.normal(size=(3, 3))) for _ in range(10)]


@functools.lru_cache(maxsize=None)
def ransac_start(model, noise, frac, seed):
    """what the parent returns for the noisy case: geometry_ref.ransac with the refits, at find_*'s defaults, on the points as
    the device reads them"""
    _, pa, pb, _, _ = scene(model, frac, noise)
    conf, iters = ((0.995, 2000), (0.99, 1000))[model]
    r = gr.ransac(model, mr.as_f32(pa), mr.as_f32(pb), noisy_thr(noise), conf, iters, seed, refine=True)
    assert r["ok"]
    return r["M"]


def noisy_thr(noise):
    return max(1.0, 2 * noise)


def clean_fits(model, f32=True):
    """(name, start, pa, pb, thr, frac, noise) of the 30 clean fits; f32: the points as the device reads them"""
    out = []
    for frac in FRACS:
        M0, pa, pb, _, _ = scene(model, frac)
        if f32:
            pa, pb = mr.as_f32(pa), mr.as_f32(pb)
        out += [(f"clean {'HF'[model]} {frac} {i}", Ms, pa, pb, CLEAN_THR[model], frac, 0.0) for i, Ms in enumerate(starts(model, M0))]
    return out


def noisy_fits(model):
    """the 24 noisy fits from the RANSAC's model, on the points as the device reads them"""
    out = []
    for noise, frac in NOISY_CASES:
        _, pa, pb, _, _ = scene(model, frac, noise)
        for seed in NOISY_SEEDS:
            out.append((f"noisy {'HF'[model]} {noise} {frac} {seed}", ransac_start(model, noise, frac, seed), mr.as_f32(pa), mr.as_f32(pb),
                        noisy_thr(noise), frac, noise))
    return out


def edge_rows(model, M, pa, pb, thr):
    """rows whose |r|^2 lies within 1e-9 relative of thr^2 under M: they may fall either way on the device"""
    w, Mn, _ = mr.prepare(model, M, pa, pb)
    fit = mr.FITS[model]
    _, r2 = mr.active(fit.residuals(fit.init(Mn), w), thr)
    with np.errstate(invalid="ignore"):
        return int((np.abs(r2 - thr * thr) < 1e-9 * thr * thr).sum())


def check_monotone(model, o, Ms, pa, pb, thr):
    """item 4: the cost never rises and `cost` is the direct evaluation of start and result"""
    assert o["cost"] <= o["cost0"] and o["info"][0] <= MAX_STEPS and o["info"][1] <= 1 + 11 * MAX_STEPS
    c0, _ = mr.pixel_cost(model, Ms, pa, pb, thr)
    c1, a1 = mr.pixel_cost(model, o["M"], pa, pb, thr)
    # the result is de-normalised and normalised again on the way, which moves each residual by rounding of coordinates of
    # 1e3 px: some 1e-12 px.  With d = 1e-10 px per residual the cost moves by at most 2 sqrt(n cost) d + n d^2.
    d, n = 1e-10, len(pa)
    assert o["cost0"] == c0 and abs(o["cost"] - c1) <= 2 * math.sqrt(n * c1) * d + n * d * d, (o["cost0"], c0, o["cost"], c1)
    assert np.array_equal(o["mask"], a1) and o["info"][2] == int(a1.sum())


# ------------------------------------------------------------------------------------------------------------ definitions
def _random_state(model, rng):
    M = np.eye(3) + 0.1 * rng.normal(size=(3, 3)) if model == H else rng.normal(size=(3, 3))
    return mr.FITS[model].init(M / np.linalg.norm(M))


@pytest.mark.parametrize("model", [H, F])
def test_jacobian_equals_central_differences(model):
    rng = np.random.default_rng(0)
    fit = mr.FITS[model]
    for _ in range(5):
        st = _random_state(model, rng)
        w = mr.Rows(*rng.uniform(-1.5, 1.5, (4, 200)), 0.0041, 0.0037)
        e, J = fit.jacobian(st, w)
        assert J.shape == (200, fit.NRES, fit.NPAR) and np.array_equal(e, fit.residuals(st, w))
        h = 1e-6
        Jn = np.zeros_like(J)
        for i in range(fit.NPAR):
            d = np.zeros(fit.NPAR)
            d[i] = h
            Jn[:, :, i] = (fit.residuals(fit.apply(st, d), w) - fit.residuals(fit.apply(st, -d), w)) / (2 * h)
        assert np.abs(J - Jn).max() <= 1e-6 * np.abs(J).max(), np.abs(J - Jn).max() / np.abs(J).max()


def test_fundamental_chart_is_the_rank_two_factorisation():
    rng = np.random.default_rng(2)
    for _ in range(5):
        M = rng.normal(size=(3, 3))
        U, V, sg = mr.svd_rank2(M / np.linalg.norm(M))
        s = np.linalg.svd(M / np.linalg.norm(M), compute_uv=False)
        assert abs(sg - s[1] / s[0]) < 1e-14
        for Q in (U, V):
            assert np.abs(Q.T @ Q - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Q) - 1) < 1e-14
        st = (U, V, sg)
        Fm = mr.FundamentalFit.matrix(st)
        assert np.abs(Fm - (U * [1, sg, 0]) @ V.T).max() < 1e-15 and abs(np.linalg.det(Fm)) < 1e-16
        # the closed-form derivative matrices against the retraction, and rank 2 after a large step
        dF = mr.FundamentalFit.derivatives(st)
        for i in range(7):
            d = np.zeros(7)
            d[i] = 1e-6
            num = (mr.FundamentalFit.matrix(mr.FundamentalFit.apply(st, d)) - mr.FundamentalFit.matrix(mr.FundamentalFit.apply(st, -d))) / 2e-6
            assert np.abs(num - dF[i]).max() < 1e-9
        assert abs(np.linalg.det(mr.FundamentalFit.matrix(mr.FundamentalFit.apply(st, rng.normal(size=7))))) < 1e-15


def test_residuals_are_the_pixel_errors():
    for model in (H, F):
        M0, pa, pb, truth, _ = scene(model, 0.3, 1.0)
        M = M0 * (1 + 1e-3 * np.random.default_rng(3).normal(size=(3, 3)))
        w, Mn, nrm = mr.prepare(model, M, pa, pb)
        fit = mr.FITS[model]
        st = fit.init(Mn)
        e = fit.residuals(st, w)
        ha, hb = np.c_[pa, np.ones(len(pa))], np.c_[pb, np.ones(len(pb))]
        if model == H:
            p = ha @ M.T
            direct = p[:, :2] / p[:, 2:] - pb
            assert np.abs(e - direct).max() <= 1e-9 * np.abs(direct).max()
        else:
            Mp = mr.denormalise(F, fit.matrix(st), *nrm)  # the rank-2 projection of M, in pixels
            assert abs(np.linalg.det(Mp)) < 1e-12 * np.linalg.norm(Mp) ** 3
            l, k = ha @ Mp.T, hb @ Mp
            direct = (hb * l).sum(1) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2 + k[:, 0] ** 2 + k[:, 1] ** 2)
            sign = np.sign((e[:, 0] * direct).sum())  # the scale of M^, so its sign, is free
            assert np.abs(e[:, 0] - sign * direct).max() <= 1e-9 * np.abs(direct).max()


# ------------------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("model", [H, F])
@pytest.mark.parametrize("frac", FRACS)
def test_exact_convergence_on_clean_data(model, frac):
    """measured with this oracle: H corner error at most 5.0e-8 px in 2 - 3 steps, F epipolar distance at most 3.2e-8 px in
    4 - 6 steps, on the scenes' f64 points (rounded to f32, as the device reads them, the points themselves are off by
    3e-5 px and the fits end 2.4e-6 / 5.0e-7 px from the truth)"""
    M0, pa, pb, truth, clean = scene(model, frac)
    thr = CLEAN_THR[model]
    for Ms in starts(model, M0):
        assert mr.pixel_cost(model, Ms, pa, pb, thr)[1].sum() >= mr.MIN_ROWS[model]
        o = mr.refine(model, Ms, pa, pb, thr, MAX_STEPS)
        err = corner_error(o["M"], M0) if model == H else epipolar_error(o["M"], *clean, reduce=np.max)
        assert err < 1e-6 and 1 <= o["info"][0] <= MAX_STEPS and o["info"][3] == 1, (err, o["info"])
        assert np.array_equal(o["mask"], truth) and o["info"][2] == int(truth.sum())
        check_monotone(model, o, Ms, pa, pb, thr)
        assert abs(o["M"][2, 2] - 1) < 1e-15
        if model == F:
            assert abs(np.linalg.det(o["M"])) < 1e-12 * np.linalg.norm(o["M"]) ** 3


@pytest.mark.parametrize("model", [H, F])
def test_clean_fits_on_device_points_are_monotone_and_have_no_edge_rows(model):
    """the 30 clean fits as the GPU test runs them (points rounded to f32): item 4, and no row at the threshold"""
    for name, Ms, pa, pb, thr, frac, noise in clean_fits(model):
        o = mr.refine(model, Ms, pa, pb, thr, MAX_STEPS)
        check_monotone(model, o, Ms, pa, pb, thr)
        assert o["info"][0] >= 1 and edge_rows(model, o["M"], pa, pb, thr) == 0, name


@pytest.mark.parametrize("model", [H, F])
def test_refinement_on_the_noisy_cases(model):
    """The point of the feature: the RANSAC's model (with its algebraic refits) against its LM fit, 24 cases per model.
    Measured with this oracle -
      F (mean epipolar distance of the noise-free inliers, px): median 0.2093 -> 0.0895, lower in 21 of 24
      H (mean corner error, px):                                median 0.0618 -> 0.0714, lower in 13 of 24
    F gains what the pose refinement gained.  H does not: the normalised DLT refit on 900 - 1 400 inliers is already within
    3e-6 relative of the geometric optimum's truncated cost, the six RANSAC seeds of a case all reach the same minimum
    (0.1236 px for 1 px noise / 30 % outliers, where they started between 0.064 and 0.180), and that minimum's distance from
    the truth is the noise draw's, not the fit's.  So the median is asserted for F; H is held to the monotone cost, and the
    figures above stand as measured."""
    before, after = [], []
    for name, Ms, pa, pb, thr, frac, noise in noisy_fits(model):
        o = mr.refine(model, Ms, pa, pb, thr, MAX_STEPS)
        check_monotone(model, o, Ms, pa, pb, thr)
        assert o["info"][3] == 1 and edge_rows(model, o["M"], pa, pb, thr) == 0, name
        before.append(error(model, Ms, frac, noise))
        after.append(error(model, o["M"], frac, noise))
        print(f"{name}: {before[-1]:.4f} -> {after[-1]:.4f} px, cost {o['cost0']:.6e} -> {o['cost']:.6e}, info {o['info']}")
    before, after = np.array(before), np.array(after)
    print(f"lower in {(after < before).sum()} of {len(after)}, median {np.median(before):.4f} -> {np.median(after):.4f}")
    if model == F:
        assert np.median(after) <= np.median(before)


@pytest.mark.parametrize("model", [H, F])
def test_degenerate_active_sets_return_the_input(model):
    """a start outside the threshold band: fewer active rows than MIN_ROWS, the input comes back with zero accepted steps"""
    M0, pa, pb, truth, _ = scene(model, 0.0)
    shift = np.eye(3)
    shift[0, 2] = 50.0  # image B moved by 50 px
    Ms = shift @ M0 if model == H else np.linalg.inv(shift).T @ M0
    thr = CLEAN_THR[model]
    act = int(mr.pixel_cost(model, Ms, pa, pb, thr)[1].sum())
    assert act < mr.MIN_ROWS[model]
    o = mr.refine(model, Ms, pa, pb, thr)
    assert np.array_equal(o["M"], Ms) and o["info"] == (0, 1, act, 1) and o["cost"] == o["cost0"]
    # not fitted at all: invalid, too few rows, a non-finite or zero model
    for kw in (dict(valid=False), ):
        o = mr.refine(model, 2 * M0, pa, pb, thr, **kw)
        assert np.array_equal(o["M"], 2 * M0) and o["info"] == (0, 0, 0, 0) and not o["mask"].any() and math.isnan(o["cost"])
    k = mr.MIN_ROWS[model] - 1
    assert mr.refine(model, M0, pa[:k], pb[:k], thr)["info"] == (0, 0, 0, 0)
    assert mr.refine(model, np.zeros((3, 3)), pa, pb, thr)["info"] == (0, 0, 0, 0)
    assert mr.refine(model, M0 * np.nan, pa, pb, thr)["info"] == (0, 0, 0, 0)
    o = mr.refine(model, 2 * M0, pa, pb, thr, max_steps=0)
    assert np.array_equal(o["M"], 2 * M0) and o["info"] == (0, 1, int(truth.sum()), 1) and np.array_equal(o["mask"], truth)


def test_infinite_threshold_is_least_squares_over_the_finite_rows():
    for model in (H, F):
        M0, pa, pb, truth, _ = scene(model, 0.0, 0.3)
        pa = pa.copy()
        pa[5] = np.nan
        o = mr.refine(model, starts(model, M0)[0], pa, pb, math.inf)
        assert o["info"][0] >= 1 and o["info"][2] == len(pa) - 1 and not o["mask"][5] and o["cost"] < o["cost0"] < math.inf
        keep = np.arange(len(pa)) != 5
        o2 = mr.refine(model, starts(model, M0)[0], pa[keep], pb[keep], math.inf)
        assert np.abs(o["M"] - o2["M"]).max() < 1e-9 * np.abs(o2["M"]).max()


def test_solver_rule():
    Hm = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 0.0])
    assert mr.solve(Hm, np.ones(8), 1e-3) is None                     # a zero pivot is not above 1e-14 x the largest diagonal
    Hm[7, 7] = 1e-3
    d = mr.solve(Hm, np.ones(8), 0.5)
    assert np.abs(d + 1 / (1.5 * np.diag(Hm))).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert len(_lib.SIGNATURES["roma_op_refine_model"][1]) == 17
    assert built_lib.roma_op_refine_model_workspace(8, 5000) > 0
    assert built_lib.roma_op_refine_model_workspace(0, 10) == 0 and built_lib.roma_op_refine_model_workspace(4, -1) == 0


def test_arguments_are_validated_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null address: validation must fail before it is used

    def call(*, model=0, M=p, a=p, out=p, cost=p, B=1, N=10, thr=1.0, steps=25, ws=p, nws=1 << 20):
        return lib.roma_op_refine_model(model, M, a, p, None, None, B, N, thr, steps, out, p, p, cost, ws, nws, None)
    for kw, word in ((dict(M=None), b"null"), (dict(a=None), b"null"), (dict(out=None), b"null"), (dict(cost=None), b"null"),
                     (dict(ws=None), b"null"), (dict(B=-1), b"B"), (dict(N=-3), b"N"), (dict(thr=0.0), b"threshold"),
                     (dict(thr=-1.0), b"threshold"), (dict(thr=float("nan")), b"threshold"), (dict(steps=-1), b"max_steps"),
                     (dict(model=2), b"model"), (dict(model=-1), b"model"), (dict(nws=16), b"workspace"),
                     (dict(nws=-5), b"workspace")):
        assert call(**kw) != 0 and word in lib.roma_last_error(), kw
    assert call(B=0, nws=0) == 0  # nothing to do, nothing launched


def test_refinement_refuses_host_tensors():
    import roma_amd
    from roma_amd import _lib
    x = torch.zeros(10, 2)
    M = torch.eye(3, dtype=torch.float64)
    calls = (lambda: roma_amd.refine_homography(M, x, x, 1.0), lambda: roma_amd.refine_fundamental(M, x, x, 1.0),
             lambda: roma_amd.find_homography(x, x, lm_steps=10), lambda: roma_amd.find_fundamental(x, x, lm_steps=10))
    for call in calls:
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            call()


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_model_refine_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "model_refine.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/model_refine.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["model_refine_kernel<FundamentalFit>", "model_refine_kernel<HomographyFit>",
                     "model_refine_mask_kernel<FundamentalFit>", "model_refine_mask_kernel<HomographyFit>"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
