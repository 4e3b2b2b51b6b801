"""The numpy oracle of the absolute pose (tools/absolute_pose_ref.py) against exact synthetic geometry, and the C ABI of
roma_op_absolute_pose / _minimal / refine_absolute_pose / lift_matches without a GPU (argument validation only)."""
import os
import re

import numpy as np
import pytest
import torch

from absolute_pose_cases import THR, ar, exact_samples, f32, pose_error, rot_angle_deg, scene, true_pose_error
from conftest import ROOT

NEW_SYMBOLS = ["roma_op_absolute_pose", "roma_op_absolute_pose_workspace", "roma_op_absolute_pose_minimal",
               "roma_op_refine_absolute_pose", "roma_op_lift_matches"]


def test_oracle_p3p_contains_the_true_pose_on_exact_samples():
    """The bar test_gpu_essential.py holds the five-point solver to: the true pose among the solutions to 1e-9 on >= 99.5 % of
    4096 exact samples, none beyond 1e-6.  This oracle (48 bisections, 3 Newton and 3 Gauss-Newton steps), seed 3: 4096 of 4096
    within 1e-9, worst 2.9e-11, median 5.3e-15; 1293 / 2323 / 138 / 342 samples with 1 / 2 / 3 / 4 solutions."""
    X, x, R, t = exact_samples(4096, seed=3)
    Rs, ts, n = ar.p3p(X, x)
    err = true_pose_error(Rs, ts, n, R, t)
    print(f"within 1e-9: {(err < 1e-9).sum()}, worst {err.max():.2e}, median {np.median(err):.2e}, solutions {np.bincount(n, minlength=5)}")
    assert (err < 1e-9).mean() >= 0.995 and (err > 1e-6).sum() == 0
    assert (np.bincount(n, minlength=5)[1:] > 0).all()  # every slot count occurs
    # every solution is a rigid motion that maps the sample onto its rays, and the slots beyond n are empty
    for s in range(4):
        use = s < n
        Y = np.einsum("mij,mkj->mki", Rs[use, s], X[use]) + ts[use, s][:, None]
        assert (Y[..., 2] > 0).all() and np.abs(Y[..., :2] / Y[..., 2:] - x[use]).max() < 1e-6
        assert np.abs(np.einsum("mij,mkj->mik", Rs[use, s], Rs[use, s]) - np.eye(3)).max() < 1e-9
        assert not Rs[~use, s].any() and not ts[~use, s].any()


def test_oracle_ransac_is_exact_on_a_clean_scene():
    K, R, t, X, kp, truth = scene(n=2000, outlier_frac=0.3)
    r = ar.ransac(X, kp, K, THR, 0.9999, 1000, seed=1)
    assert r["ok"] and np.array_equal(r["mask"], truth) and r["best"] == truth.sum()
    assert pose_error(r["R"], r["t"], R, t) < 1e-9
    Rr, tr, mask = ar.estimate_absolute_pose(X, kp, K, THR, seed=1)
    assert np.array_equal(mask, truth) and pose_error(Rr, tr[:, 0], R, t) < 1e-9 and tr.shape == (3, 1)


def noisy_fits():
    """(rotation error in degrees, translation error) of the winning minimal sample and of the LM-refined pose on the eight
    0.5 px scenes"""
    out = []
    for seed in range(8):
        K, R, t, X, kp, truth = scene(n=2000, outlier_frac=0.3, noise_px=0.5, rng_seed=10 + seed)
        X, kp = f32(X), f32(kp)
        r = ar.ransac(X, kp, K, THR, 0.9999, 1000, seed)
        o = ar.refine(r["R"], r["t"], X, kp, K, THR)
        assert r["ok"] and o["info"][3] == 1 and o["cost"] <= o["cost0"]
        out.append((rot_angle_deg(r["R"], R), np.linalg.norm(r["t"] - t), rot_angle_deg(o["R"], R), np.linalg.norm(o["t"] - t)))
    return np.array(out)


def test_oracle_refinement_improves_the_noisy_scenes():
    e = noisy_fits()
    med = np.median(e, axis=0)
    print(f"median rotation error {med[0]:.4f} -> {med[2]:.4f} degrees, translation error {med[1]:.5f} -> {med[3]:.5f}")
    assert med[2] <= med[0] and med[3] <= med[1]


def test_oracle_degenerate_input_gives_no_model():
    rng = np.random.default_rng(0)
    K, R, t, X, kp, truth = scene(n=300, outlier_frac=0.0)
    line = X[0] + np.linspace(0, 1, 300)[:, None] * (X[1] - X[0])           # collinear 3-D points, whatever the pixels
    same = np.repeat(X[:1], 300, axis=0)                                     # all points identical
    few = X.copy()
    few[3:] = np.nan                                                         # fewer than 4 finite rows
    # every point behind the camera (identity pose).  A sample's three rows still have a solution with positive depths - the
    # triangle reflected through the centre - which fits a fourth row only where that row lies in the triangle's plane: eight
    # points in general position leave no such row, a dense cloud would offer some within a pixel
    Xc = rng.uniform([-2, -2, -8], [2, 2, -2], (8, 3))
    kc = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
    for name, Xd, kd in (("collinear", line, kp), ("identical", same, kp), ("few", few, kp), ("behind", Xc, kc)):
        r = ar.ransac(Xd, kd, K, THR, 0.9999, 512, seed=2)
        assert not r["ok"] and not r["mask"].any() and not r["R"].any() and not r["t"].any(), name
        assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()
        assert ar.estimate_absolute_pose(Xd, kd, K, THR, max_iters=512, seed=2) is None
    # rows of a valid pair that hold NaN are never inliers and the pose is that of the finite rows
    K, R, t, X, kp, truth = scene(n=400, outlier_frac=0.2)
    X[::7] = np.nan
    r = ar.ransac(X, kp, K, THR, 0.9999, 512, seed=3)
    assert r["ok"] and not r["mask"][::7].any() and pose_error(r["R"], r["t"], R, t) < 1e-9


def test_abi_symbols_and_sources(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [18, 2, 7, 16, 12]
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "absolute_pose.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "absolute_pose" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()
    ws = built_lib.roma_op_absolute_pose_workspace
    assert ws(0, 100) == 0 and ws(4, 0) == 0 and 0 < ws(1, 100) < ws(1, 1000) < ws(8, 1000)
    assert ws(8, 1000) - ws(8, 100) >= 8 * 900 * 24  # a float4 and a float2 per row


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    need = lib.roma_op_absolute_pose_workspace(2, 100)

    def pose(points=p, B=2, N=100, thr=1.0, conf=0.99, iters=100, ws=p, nws=need):
        return lib.roma_op_absolute_pose(points, p, None, p, None, B, N, thr, conf, iters, p, p, p, p, p, ws, nws, None)

    def refine(R=p, B=2, N=100, thr=1.0, steps=5):
        return lib.roma_op_refine_absolute_pose(R, p, p, p, None, None, None, B, N, thr, steps, p, p, p, p, None)

    def lift(m=p, B=2, N=100, H=9, W=13, HB=9, WB=13):
        return lib.roma_op_lift_matches(m, p, p, B, N, H, W, HB, WB, p, p, None)

    cases = [(lambda: pose(points=None), "null pointer"), (lambda: pose(ws=None), "null pointer"),
             (lambda: pose(B=0), "0 < B"), (lambda: pose(N=-1), "0 < N"),
             (lambda: pose(thr=0.0), "threshold"), (lambda: pose(thr=float("nan")), "threshold"),
             (lambda: pose(conf=1.5), "conf"), (lambda: pose(conf=-0.1), "conf"),
             (lambda: pose(iters=0), "max_iters"), (lambda: pose(nws=need - 1), "workspace too small"),
             (lambda: lib.roma_op_absolute_pose_minimal(None, p, 4, p, p, p, None), "null pointer"),
             (lambda: lib.roma_op_absolute_pose_minimal(p, p, 0, p, p, p, None), "0 < S"),
             (lambda: refine(R=None), "null pointer"), (lambda: refine(B=0), "0 < B"), (lambda: refine(N=0), "0 < N"),
             (lambda: refine(thr=-1.0), "threshold"), (lambda: refine(thr=float("inf")), "threshold"),
             (lambda: refine(steps=-1), "max_steps"),
             (lambda: lift(m=None), "null pointer"), (lambda: lift(B=-2), "0 < B"), (lambda: lift(N=0), "0 < N"),
             (lambda: lift(H=0), "image sizes"), (lambda: lift(WB=0), "image sizes")]
    for call, word in cases:
        assert call() != 0 and word in lib.roma_last_error().decode(), (word, lib.roma_last_error())


def test_python_functions_refuse_host_tensors(built_lib):
    import roma_amd
    from roma_amd import RegressionMatcher
    from roma_amd._lib import RomaHipError
    X, x, K = torch.zeros(8, 3), torch.zeros(8, 2), np.eye(3)
    calls = [lambda: roma_amd.estimate_absolute_pose(X, x, K), lambda: roma_amd.absolute_pose.absolute_pose(X[None], x[None], K),
             lambda: roma_amd.refine_absolute_pose(torch.eye(3), torch.zeros(3, 1), X, x, K, 1.0),
             lambda: roma_amd.absolute_pose_minimal(torch.zeros(2, 3, 3, dtype=torch.float64), torch.zeros(2, 3, 2, dtype=torch.float64)),
             lambda: roma_amd.lift_matches(torch.zeros(8, 4), torch.ones(9, 13), K, 9, 13),
             lambda: RegressionMatcher.localize(None, torch.zeros(8, 4), torch.ones(9, 13), K, K, 9, 13)]
    for call in calls:
        with pytest.raises(RomaHipError, match="no CPU fallback"):
            call()
