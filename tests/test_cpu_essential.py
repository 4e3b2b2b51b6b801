"""tools/essential_ref.py (the oracle of the device essential-matrix RANSAC and recoverPose) on exact synthetic geometry, and the
C ABI of roma_op_essential / roma_op_recover_pose / roma_op_essential_minimal (dlopen only).  No GPU."""
import glob
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

NEW_SYMBOLS = ("roma_op_essential", "roma_op_essential_workspace", "roma_op_essential_minimal", "roma_op_recover_pose",
               "roma_op_recover_pose_workspace")


def _rot(rng, max_angle=0.5):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.05, max_angle)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * k @ k


def exact_samples(S, seed=0):
    """S exact five-point samples (normalised points of a random scene 3 .. 8 units deep) and their true E (unit norm, the
    sign rule of the solver)"""
    rng = np.random.default_rng(seed)
    x0, x1, Es = [], [], []
    for _ in range(S):
        R = _rot(rng)
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = np.c_[rng.uniform(-1, 1, (5, 2)), rng.uniform(3, 8, 5)]
        X[:, :2] *= X[:, 2:]
        Y = X @ R.T + t
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        E = tx @ R
        E /= np.linalg.norm(E)
        E *= np.sign(E.flat[np.argmax(np.abs(E))])
        x0.append(X[:, :2] / X[:, 2:])
        x1.append(Y[:, :2] / Y[:, 2:])
        Es.append(E)
    return np.array(x0), np.array(x1), np.array(Es)


def true_root_error(E, n, Et):
    """per sample: the smallest max-abs difference between a returned root and the true E"""
    return np.array([np.abs(E[i, :n[i]] - Et[i]).max(axis=(1, 2)).min() if n[i] else np.inf for i in range(len(n))])


def test_five_point_solver_finds_the_true_essential_matrix():
    x0, x1, Et = exact_samples(400)
    E, n = er.five_point(x0, x1)
    assert n.max() <= er.MAX_ROOTS and (n % 2 == 0).all()  # real roots of a degree-10 polynomial come in an even count here
    err = true_root_error(E, n, Et)
    # the true E to 1e-9 on >= 99.5 % of exact samples; a miss beyond 1e-6 is a sample whose Sturm chain loses a root (about
    # 1 in 1 000): at most 1 of these 400
    assert (err < 1e-9).mean() >= 0.995 and (err > 1e-6).sum() <= 1, (np.percentile(err, [50, 99.5]), np.sort(err)[-3:])


def test_five_point_roots_satisfy_the_essential_constraints():
    x0, x1, _ = exact_samples(200, seed=1)
    E, n = er.five_point(x0, x1)
    a0 = np.concatenate([x0, np.ones((len(x0), 5, 1))], 2)
    a1 = np.concatenate([x1, np.ones((len(x1), 5, 1))], 2)
    res = []
    for i in range(len(n)):
        for r in range(n[i]):
            e = E[i, r]
            assert abs(np.linalg.norm(e) - 1) < 1e-12 and e.flat[np.argmax(np.abs(e))] > 0
            res.append(max(np.abs(np.einsum("ki,ij,kj->k", a1[i], e, a0[i])).max(), abs(np.linalg.det(e)),
                           np.abs(2 * e @ e.T @ e - np.trace(e @ e.T) * e).max()))
        assert (E[i, n[i]:] == 0).all()
    res = np.array(res)
    assert (res < 1e-9).mean() >= 0.995, (np.percentile(res, [50, 99.5]), np.sort(res)[-3:])


def test_five_point_rejects_a_degenerate_sample():
    s = np.linspace(-1, 1, 5)
    line = np.stack([s, 0.5 * s + 0.1], 1)[None]
    assert er.five_point(line, 2 * line)[1][0] == 0


@pytest.mark.parametrize("frac", [0.3, 0.5])
def test_reference_ransac_and_recover_pose_on_relief_scene(frac):
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, outlier_frac=frac)
    Rp, tp, mask = er.estimate_pose(pa, pb, K, K, 0.5 / K[0, 0], 0.99999, 1000, seed=1)
    e_t, e_R = pg.compute_pose_error(np.c_[R, t], Rp, tp)
    assert e_t < 0.5 and e_R < 0.5, (e_t, e_R)
    assert np.array_equal(mask, truth)  # outliers are far from the threshold; every inlier is in front of both cameras
    h = pg.estimate_pose(pa, pb, K, K, 0.5 / K[0, 0], 0.99999, rng=np.random.default_rng(0))
    h_t, h_R = pg.compute_pose_error(np.c_[R, t], h[0], h[1])
    assert h_t < 1.0 and h_R < 0.5 and pg.angle_error_mat(Rp, h[0]) < 0.5


def test_reference_recover_pose_matches_pose_geometry_on_exact_E():
    K, R, t, F, pa, pb, truth = relief_scene(n=800, outlier_frac=0.0)
    Ki = np.linalg.inv(K)
    x0, x1 = (np.c_[pa, np.ones(len(pa))] @ Ki.T)[:, :2], (np.c_[pb, np.ones(len(pb))] @ Ki.T)[:, :2]
    E = K.T @ F @ K
    n, Rp, tp, m = er.recover_pose(E, x0, x1)
    n2, R2, t2, m2 = pg.recover_pose(E, x0, x1, np.ones(len(x0), dtype=bool))
    assert n == n2 == len(x0) and np.array_equal(m, m2)
    assert np.abs(Rp - R2).max() < 1e-9 and np.abs(tp - t2).max() < 1e-9
    assert np.abs(Rp - R).max() < 1e-6 and np.abs(tp[:, 0] - t / np.linalg.norm(t)).max() < 1e-6


def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert built_lib.roma_op_essential_workspace(8, 5000) > 8 * 5000 * 16
    assert built_lib.roma_op_recover_pose_workspace(8, 5000) > 8 * 5000
    assert built_lib.roma_op_essential_workspace(0, 10) == 0


def test_arguments_are_validated_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null address: validation must fail before it is used

    def ess(*, a=p, seeds=p, B=1, N=10, thr=1.0, prob=0.99, iters=100, ws=p, nws=1 << 30):
        return lib.roma_op_essential(a, p, None, seeds, None, B, N, thr, prob, iters, p, p, p, p, ws, nws, None)
    for kw, word in ((dict(a=None), b"null"), (dict(seeds=None), b"null"), (dict(B=0), b"B"), (dict(N=0), b"N"),
                     (dict(thr=0.0), b"threshold"), (dict(thr=float("nan")), b"threshold"), (dict(prob=1.5), b"prob"),
                     (dict(iters=0), b"max_iters"), (dict(nws=16), b"workspace")):
        assert ess(**kw) != 0 and word in lib.roma_last_error(), kw
    assert lib.roma_op_recover_pose(None, p, p, None, None, None, 1, 10, 1e9, p, p, p, p, p, 1 << 30, None) != 0
    assert b"null" in lib.roma_last_error()
    assert lib.roma_op_recover_pose(p, p, p, None, None, None, 0, 10, 1e9, p, p, p, p, p, 1 << 30, None) != 0
    assert lib.roma_op_recover_pose(p, p, p, None, None, None, 1, 10, 0.0, p, p, p, p, p, 1 << 30, None) != 0
    assert b"distance_thresh" in lib.roma_last_error()
    assert lib.roma_op_essential_minimal(None, p, 1, p, p, None) != 0 and b"null" in lib.roma_last_error()
    assert lib.roma_op_essential_minimal(p, p, 0, p, p, None) != 0


def test_pose_functions_refuse_host_tensors():
    import roma_amd
    from roma_amd import _lib
    x = torch.zeros(10, 2)
    K = torch.eye(3, dtype=torch.float64)
    calls = (lambda: roma_amd.find_essential(x, x), lambda: roma_amd.recover_pose(torch.eye(3), x, x),
             lambda: roma_amd.estimate_pose(x, x, K, K, 1e-3), lambda: roma_amd.estimate_pose_uncalibrated(x, x, K, K, 1.0),
             lambda: roma_amd.essential_minimal(torch.zeros(4, 5, 2), torch.zeros(4, 5, 2)))
    for call in calls:
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            call()


# the 7-point hypothesis kernel keeps its three f64 models in private memory (224 bytes a lane); that figure must not grow
SCRATCH_ALLOWED = {"ransac_hyp_kernel<roma::(anonymous namespace)::Fundamental>": 224}


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_essential_kernels_have_no_spills_and_no_scratch(build):
    """the RANSAC kernels live in both objects: the shared pipeline is instantiated next to each model's policy"""
    objs = {f: os.path.join(ROOT, "roma_amd", "csrc", build, f) for f in ("geometry.o", "essential.o")}
    for f, obj in objs.items():
        if not glob.glob(obj):
            pytest.skip(f"{build}/{f} not built")
    import kernel_resources
    ks = {f: kernel_resources.kernels(obj) for f, obj in objs.items()}
    assert len(ks["geometry.o"]) >= 16 and len(ks["essential.o"]) >= 10
    seen = set()
    for k in ks["geometry.o"] + ks["essential.o"]:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0, k
        allowed = [v for name, v in SCRATCH_ALLOWED.items() if k["name"].endswith(name)]
        seen.update(name for name in SCRATCH_ALLOWED if k["name"].endswith(name))
        assert k["scratch"] <= (allowed[0] if allowed else 0), k
    assert seen == set(SCRATCH_ALLOWED)
