"""The numpy oracle of the registration operators - tools/registration_ref.py - against an independent route (SVD Umeyama through
numpy.linalg.svd), exact geometry and a hand-made case; the margins of every scene that the GPU file compares; and, without a
GPU, the C ABI of include/roma_hip_registration.h: its table, its exports, its call sites, its refusals, its kernels' resources."""
import ast
import glob
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from registration_cases import (AGREEMENT, NOISE_REL, REFINE_SEEDS, agreement_scene, collinear_samples, depth_case, exact_samples, f32, model_error, planar_scene,
                                ragged_batch, random_samples, residual, rotation, rr, scene, trajectory_case, triangle_ratio, umeyama_svd)

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_goldens import abi_classes  # noqa: E402
from roma_amd import _lib  # noqa: E402

NEW_SYMBOLS = ["roma_op_align_points_workspace", "roma_op_align_points", "roma_op_similarity_minimal", "roma_op_refine_similarity",
               "roma_op_apply_similarity", "roma_op_depth_rows", "roma_op_trajectory_error"]
EDGE = 1e-9  # no refinement decision of a GPU scene may lie within this (relative) of its boundary


def _fit(X, Y, with_scale=True):
    o = rr.fit_similarity(X, Y, with_scale)
    assert o["info"] == (1, 2, len(X), 1)
    return o["s"], o["R"], o["t"]


@pytest.mark.parametrize("with_scale", [True, False])
def test_closed_form_is_svd_umeyama(with_scale):
    """the same rows through Horn's quaternion by Jacobi and through numpy's SVD: noisy, far from any exact similarity"""
    g = np.random.default_rng(0)
    for k in range(20):
        n = int(g.integers(3, 200))
        X = g.normal(size=(n, 3)) * g.uniform(0.1, 10, 3) + g.uniform(-50, 50, 3)
        Y = g.uniform(0.2, 5) * X @ rotation(g).T + g.uniform(-50, 50, 3) + g.normal(size=(n, 3)) * g.uniform(0, 2)
        s, R, t = _fit(X, Y, with_scale)
        s0, R0, t0 = umeyama_svd(X, Y, with_scale)
        assert model_error(s, R, t, s0, R0, t0) < 1e-10, (k, n)
        assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        if not with_scale:
            assert s == 1.0


def test_mirrored_set_still_gives_a_proper_rotation():
    """dst is a reflection of src: the best ROTATION is what Umeyama's sign correction picks, never det = -1"""
    g = np.random.default_rng(1)
    X = g.normal(size=(60, 3)) * [3.0, 2.0, 1.0]
    Y = (X * [1.0, 1.0, -1.0]) @ rotation(g).T + [1.0, 2.0, 3.0]
    s, R, t = _fit(X, Y)
    s0, R0, t0 = umeyama_svd(X, Y)
    assert abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.det(R0) - 1) < 1e-12
    assert model_error(s, R, t, s0, R0, t0) < 1e-10


def test_exact_recovery_and_the_minimal_solver():
    X, Y, s, R, t = exact_samples(2048, seed=3)
    assert triangle_ratio(X).min() >= 0.2
    sm, Rm, tm, n = rr.minimal(X, Y)
    assert n.all() and model_error(sm, Rm, tm, s, R, t).max() < 1e-12
    sm, Rm, tm, n = rr.minimal(X, Y / s[:, None, None], with_scale=False)  # a rigid pair
    assert n.all() and (sm == 1.0).all() and np.abs(Rm - R).max() < 1e-12
    Xc, Yc = collinear_samples(512, seed=4)
    sm, Rm, tm, n = rr.minimal(Xc, Yc)
    assert not n.any() and not sm.any() and not Rm.any() and not tm.any()
    Xr, Yr = random_samples(512, seed=5)
    sm, Rm, tm, n = rr.minimal(Xr, Yr)
    assert n.all()
    for i in range(0, 512, 37):  # the least-squares similarity of two unrelated triangles is SVD Umeyama's as well
        assert model_error(sm[i], Rm[i], tm[i], *umeyama_svd(Xr[i], Yr[i])) < 1e-9, i
    # noise-free scenes: plain fit, planar source, a far origin
    Xs, Ys, _, far, _ = scene(500, 0.0, 2.9, rng_seed=5, shift=True)
    assert model_error(*_fit(Xs, Ys), *far) < 1e-3  # the noise of the scene and the f32 rounding of coordinates of 2e3, at |t| 1e4
    Xp, Yp, truth = planar_scene()
    assert model_error(*_fit(Xp, Yp), *truth) < 1e-6  # the f32 rounding of the rows
    sp, Rp, tp = _fit(Xp, Yp)
    assert np.abs(residual((sp, Rp, tp), Xp, Yp)).max() < 1e-6


def test_hand_made_four_points():
    """the corners of the unit simplex turned by 90 degrees about z, doubled and moved by (1, 2, 3)"""
    X = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    Y = np.array([[1.0, 2, 3], [1, 4, 3], [-1, 2, 3], [1, 2, 5]])
    s, R, t = _fit(X, Y)
    assert abs(s - 2) < 1e-14 and np.abs(R - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() < 1e-14 and np.abs(t - [1, 2, 3]).max() < 1e-14
    s, R, t = _fit(X, Y, with_scale=False)  # rigid: the same rotation, the centroids matched
    assert s == 1.0 and np.abs(R - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() < 1e-14
    assert np.abs(t - (Y.mean(axis=0) - R @ X.mean(axis=0))).max() < 1e-14
    # three of them are a minimal sample; two rows, or three on a line, give nothing
    assert rr.minimal(X[None, :3], Y[None, :3])[3][0] == 1
    assert rr.fit_similarity(X[:2], Y[:2])["info"][0] == 0
    line = np.array([[0.0, 0, 0], [1, 1, 1], [3, 3, 3], [-2, -2, -2]])
    assert rr.fit_similarity(line, 2 * line)["info"] == (0, 1, 0, 1)


def test_apply_composes_and_the_camera_rule_reprojects():
    g = np.random.default_rng(2)
    X = f32(g.normal(size=(100, 3)) + [0, 0, 6.0])
    s, R, t = 1.7, rotation(g), g.uniform(-2, 2, 3)
    Y = f32(s * X @ R.T + t)
    fs, fR, ft = _fit(X, Y)
    moved = rr.apply_points(fs, fR, ft, X)
    assert moved.dtype == np.float32 and np.abs(moved - Y).max() < 2e-6  # f32 rounding of coordinates below 16
    nan = X.copy()
    nan[3] = np.nan
    assert np.isnan(rr.apply_points(fs, fR, ft, nan)[3]).all()
    # cameras that see X: after the move they see s R X + t at the same pixels, at s times the depth
    cam_R = np.stack([rotation(g, 0.3) for _ in range(5)])
    cam_t = g.uniform(-0.5, 0.5, (5, 3))
    Rn, tn = rr.apply_cameras(s, R, t, cam_R, cam_t)
    Xm = s * X @ R.T + t
    for v in range(5):
        before, after = X @ cam_R[v].T + cam_t[v], Xm @ Rn[v].T + tn[v]
        assert np.abs(after - s * before).max() < 1e-12
        assert np.abs(after[:, :2] / after[:, 2:] - before[:, :2] / before[:, 2:]).max() < 1e-13
        assert np.abs(Rn[v] @ Rn[v].T - np.eye(3)).max() < 1e-14


def _no_decision_on_the_edge(decisions):
    for kind, a, b in decisions:
        if kind == "rows":  # squared residuals against the squared threshold
            assert (np.abs(a / b - 1) > EDGE).all()
        else:  # candidate cost against the current one: clear of it, or bit-equal (the same active rows give the same model)
            assert a == b or abs(a - b) > EDGE * min(a, b), (a, b)


@pytest.mark.parametrize("case", AGREEMENT, ids=lambda c: "-".join(str(v) for v in c))
def test_gpu_scenes_through_the_reference(case):
    X, Y, truth, (s, R, t), thr = agreement_scene(*case)
    for seed in ((case[1],)):
        r = rr.ransac(X, Y, thr, seed=seed)
        assert r["ok"] and r["valid"] and r["best"] >= 0.5 * truth.sum() and not r["mask"][~truth].any()
        dec = []
        o = rr.refine((r["s"], r["R"], r["t"]), X, Y, thr, decisions=dec)
        assert o["info"][0] >= 1 and o["info"][3] == 1 and o["cost"] < o["cost0"]
        _no_decision_on_the_edge(dec)
        # the refined model holds every true inlier and no outlier, and is the scene's to within one sigma of the noise of a single
        # coordinate (the fit of a thousand rows averages it down by far more; the lever of the centroid, at 4 from the origin,
        # gives some of that back), plus the f32 rounding of coordinates of 2e3 where the origin is far
        assert np.array_equal(o["mask"], truth)
        assert model_error(o["s"], o["R"], o["t"], s, R, t) < NOISE_REL * thr + (2.5e-4 if case[3] else 0.0)


@pytest.mark.parametrize("seed", REFINE_SEEDS)
def test_refinement_scenes_through_the_reference(seed):
    X, Y, truth, model, thr = scene(2000, 0.3, 2.9, rng_seed=10 + seed)
    r = rr.ransac(X, Y, thr, seed=seed)
    dec = []
    o = rr.refine((r["s"], r["R"], r["t"]), X, Y, thr, decisions=dec)
    assert r["ok"] and o["info"][0] >= 1 and np.array_equal(o["mask"], truth)
    _no_decision_on_the_edge(dec)
    # the fit of the true inliers alone is where the loop ends
    assert model_error(o["s"], o["R"], o["t"], *umeyama_svd(X[truth], Y[truth])) < 1e-9
    # without truncation: one step, every row - plain Umeyama, outliers included
    f = rr.fit_similarity(X, Y)
    assert f["info"] == (1, 2, 2000, 1) and model_error(f["s"], f["R"], f["t"], *umeyama_svd(X, Y)) < 1e-9


def test_ragged_batch_depth_rows_and_trajectory_through_the_reference():
    Xs, Ys, thr = ragged_batch(np.nan)
    for b, c in enumerate([0, 3, 4, 63, 65, 257]):
        r = rr.ransac(Xs[b, :c], Ys[b, :c], thr, 1.0, 256, seed=31 + b)
        assert r["ok"] == (c >= 4) and r["valid"] == (c >= 4), (b, c)
    d = depth_case()
    for step in (1, 3):
        src, dst = rr.depth_rows(d["da"], d["db"], d["K"], d["Ra"], d["ta"], d["Rb"], d["tb"], step)
        assert src.shape == (math.ceil(37 / step) * math.ceil(53 / step), 3) and src.dtype == np.float32
        nan = np.isnan(src).any(axis=1)
        assert np.array_equal(nan, np.isnan(dst).any(axis=1)) and 0 < nan.sum() < 0.1 * len(src)
        assert residual(d["sim"], src[~nan].astype(np.float64), dst[~nan].astype(np.float64)).max() < 2e-5
    for V in (3, 8):
        R, t, Rg, tg, sim = trajectory_case(V, seed=V)
        ok = np.ones(V, dtype=bool)
        ok[1] = V == 3  # one view masked out where more than three are left
        e = rr.trajectory_error(R, t, Rg, tg, ok)
        assert e["ok"] and abs(e["s"] - sim[0]) < 0.05 * sim[0] and e["rmse"] < 0.05 and (e["rot_err_deg"] < 3.0).all()
        assert np.isfinite(e["centre_err"]).all()
    R, t, Rg, tg, _ = trajectory_case(5, seed=9, collinear=True)
    e = rr.trajectory_error(R, t, Rg, tg)
    assert not e["ok"] and math.isnan(e["rmse"]) and np.isnan(e["centre_err"]).all() and np.isnan(e["R"]).all()
    assert not rr.trajectory_error(R[:2], t[:2], Rg[:2], tg[:2])["ok"]


# ------------------------------------------------------------------------------------------------------------ the C ABI, no GPU
def test_header_table_is_its_golden_and_the_first_table_is_untouched():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_signatures_registration.json")))
    got = abi_classes(_lib.EXTENSIONS)
    assert sorted(got) == sorted(golden) == sorted(NEW_SYMBOLS)
    for name in golden:
        assert got[name] == golden[name], name
    assert len(_lib.SIGNATURES) == 120 and not set(_lib.SIGNATURES) & set(_lib.EXTENSIONS)
    header = open(os.path.join(ROOT, "include", "roma_hip_registration.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert set(re.findall(r"\b(roma_[a-z0-9_]+)\s*\(", code)) == set(NEW_SYMBOLS)
    assert not any(n in open(os.path.join(ROOT, "include", "roma_hip.h")).read() for n in NEW_SYMBOLS)
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "registration.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "registration" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()
    src = open(os.path.join(ROOT, "roma_amd", "csrc", "registration.hip")).read()
    assert '#include "../../include/roma_hip_registration.h"' in src  # the compiler holds the definitions to the declarations


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_every_declared_name(fmt):
    lib = _lib.load(fmt)  # binds every name of both tables, AttributeError on a missing one
    for name, (res, args) in _lib.EXTENSIONS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    ws = lib.roma_op_align_points_workspace
    assert ws(0, 100) == 0 and ws(4, 0) == 0 and 0 < ws(1, 100) < ws(1, 1000) < ws(8, 1000)
    assert ws(8, 1000) - ws(8, 100) >= 8 * 900 * 32  # two float4 per row


def test_every_call_site_passes_the_declared_number_of_arguments():
    files = []
    for d in ("roma_amd", "tools"):
        files += sorted(glob.glob(os.path.join(ROOT, d, "*.py")))
    bad, seen = [], set()
    for f in files:
        for node in ast.walk(ast.parse(open(f).read(), f)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in _lib.EXTENSIONS:
                if any(isinstance(a, ast.Starred) for a in node.args):
                    continue
                seen.add(node.func.attr)
                want = len(_lib.EXTENSIONS[node.func.attr][1])
                if len(node.args) != want or node.keywords:
                    bad.append(f"{os.path.relpath(f, ROOT)}:{node.lineno} {node.func.attr}: {len(node.args)} arguments, declared {want}")
    assert seen == set(NEW_SYMBOLS) and not bad, (bad, set(NEW_SYMBOLS) - seen)


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    need = lib.roma_op_align_points_workspace(2, 100)
    inf = math.inf

    def align(src=p, B=2, N=100, thr=1.0, conf=0.99, iters=100, ws_=1, ws=p, nws=need):
        return lib.roma_op_align_points(src, p, None, p, B, N, thr, conf, iters, ws_, p, p, p, p, p, p, ws, nws, None)

    def refine(s=p, R=p, t=p, src=p, B=2, N=100, thr=1.0, steps=5, ws_=1, cost=p):
        return lib.roma_op_refine_similarity(s, R, t, src, p, None, None, B, N, thr, steps, ws_, p, p, p, p, p, cost, None)

    def apply(s=p, pts=p, N=10, cR=p, ct=p, V=3, B=2, op=p, oR=p, ot=p):
        return lib.roma_op_apply_similarity(s, p, p, pts, N, cR, ct, V, B, op, oR, ot, None)

    def rows(da=p, B=2, H=9, W=13, step=2):
        return lib.roma_op_depth_rows(da, p, p, p, p, p, p, B, H, W, step, p, p, None)

    def traj(R=p, B=2, V=4, ws_=1):
        return lib.roma_op_trajectory_error(R, p, p, p, None, B, V, ws_, p, p, p, p, p, p, None)

    cases = [(lambda: align(src=None), "align_points: null pointer"), (lambda: align(ws=None), "null pointer"), (lambda: align(B=0), "0 < B"),
             (lambda: align(N=-1), "0 < N"), (lambda: align(thr=0.0), "threshold"), (lambda: align(thr=math.nan), "threshold"),
             (lambda: align(thr=inf), "threshold"), (lambda: align(conf=1.5), "conf"), (lambda: align(iters=0), "max_iters"),
             (lambda: align(nws=need - 1), "workspace too small (roma_op_align_points_workspace)"), (lambda: align(ws_=2), "with_scale"),
             (lambda: lib.roma_op_similarity_minimal(None, p, 4, 1, p, p, p, p, None), "similarity_minimal: null pointer"),
             (lambda: lib.roma_op_similarity_minimal(p, p, 0, 1, p, p, p, p, None), "0 < S"),
             (lambda: lib.roma_op_similarity_minimal(p, p, 4, -1, p, p, p, p, None), "with_scale"),
             (lambda: refine(src=None), "refine_similarity: null pointer"), (lambda: refine(cost=None), "null pointer"),
             (lambda: refine(s=None), "go together"), (lambda: refine(R=None, t=None), "go together"), (lambda: refine(B=0), "0 < B"),
             (lambda: refine(N=0), "0 < N"), (lambda: refine(thr=-1.0), "threshold"), (lambda: refine(thr=math.nan), "threshold"),
             (lambda: refine(steps=-1), "max_steps"), (lambda: refine(ws_=3), "with_scale"),
             (lambda: apply(s=None), "apply_similarity: null pointer"), (lambda: apply(B=0), "0 < B"), (lambda: apply(N=-1), "0 <= N"),
             (lambda: apply(pts=None), "go with N > 0"), (lambda: apply(N=0), "go with N > 0"), (lambda: apply(cR=None), "go with V > 0"),
             (lambda: apply(V=0), "go with V > 0"),
             (lambda: rows(da=None), "depth_rows: null pointer"), (lambda: rows(B=0), "0 < B"), (lambda: rows(H=0), "image sizes"),
             (lambda: rows(step=0), "step"), (lambda: rows(B=4, H=30000, W=30000), "2^31"),
             (lambda: traj(R=None), "trajectory_error: null pointer"), (lambda: traj(B=0), "0 < B"), (lambda: traj(V=0), "0 < V"),
             (lambda: traj(ws_=2), "with_scale")]
    for k, (call, word) in enumerate(cases):
        assert call() != 0 and word in lib.roma_last_error().decode(), (k, word, lib.roma_last_error())


def test_python_functions_check_arguments_and_refuse_host_tensors(built_lib):
    import roma_amd
    from roma_amd._lib import RomaHipError
    X, E, z = torch.zeros(8, 3), torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    one = torch.ones((), dtype=torch.float64)
    calls = [lambda: roma_amd.align_points(X, X, 0.1), lambda: roma_amd.refine_similarity((one, E, z), X, X, 0.1),
             lambda: roma_amd.refine_similarity(None, X, X, 0.1), lambda: roma_amd.fit_similarity(X, X),
             lambda: roma_amd.similarity_minimal(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3)),
             lambda: roma_amd.apply_similarity((one, E, z), points=X), lambda: roma_amd.depth_rows(torch.ones(9, 13), torch.ones(9, 13), E, (E, z), (E, z)),
             lambda: roma_amd.register_depth_maps(torch.ones(9, 13), torch.ones(9, 13), E, (E, z), (E, z), 0.1),
             lambda: roma_amd.trajectory_error(E.expand(4, 3, 3), torch.zeros(4, 3), E.expand(4, 3, 3), torch.zeros(4, 3))]
    for k, call in enumerate(calls):
        with pytest.raises(RomaHipError, match=r"roma_amd\.registration: .* must be a tensor on a HIP device; there is no CPU fallback"):
            call()
    for name in ("Similarity", "TrajectoryError", "align_points", "similarity_minimal", "refine_similarity", "fit_similarity", "apply_similarity",
                 "depth_rows", "register_depth_maps", "trajectory_error"):
        assert name in roma_amd.__all__ and hasattr(roma_amd, name)
    assert roma_amd.Similarity._fields == ("scale", "R", "t", "mask", "ok", "info")


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_registration_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "registration.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/registration.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::|<.*", "", k["name"]) for k in ks)
    assert names == ["depth_rows_kernel", "ransac_finish_kernel", "ransac_hyp_kernel", "ransac_mask_kernel", "ransac_norm_kernel",
                     "ransac_score_kernel", "ransac_select_kernel", "sim3_apply_cameras_kernel", "sim3_apply_points_kernel",
                     "sim3_minimal_kernel", "sim3_refine_kernel", "sim3_trajectory_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        if "ransac_hyp_kernel" in k["name"]:
            assert k["vgpr"] <= 128, k  # four waves a SIMD with one lane per hypothesis: the f64 Jacobi stays in registers
        if "sim3_refine_kernel" in k["name"] or "sim3_trajectory_kernel" in k["name"]:
            assert k["vgpr"] <= 256, k  # LM_THREADS = 512: two waves a SIMD
