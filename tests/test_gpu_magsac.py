"""Device MAGSAC++ (roma_amd.geometry.magsac, find_homography / find_fundamental(method="magsac"), csrc/ransac.h magsac_*)
against its numpy restatement tools/magsac_ref.py, its accuracy against the device RANSAC where matches are wrong by a few
pixels, batching, determinism, degenerate input, and the demo_fundamental pipeline end to end."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_geometry import _homography_scene, epipolar_dist, relief_scene
from test_cpu_magsac import F_ARGS, H_ARGS, SCENES, corner_error, f_error, f_local_scene, h_local_scene

sys.path.insert(0, os.path.join(ROOT, "tools"))
import geometry_ref as gr  # noqa: E402
import magsac_ref as mr  # noqa: E402
import pose_geometry as pg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REL_R = 1e-4   # relative error of an f32 residual the agreement tests grant (tests/test_gpu_geometry.py grants it at the threshold)
MARGIN = 10    # device / oracle margin over the oracle's own f32 sensitivity (the pose-refinement tests use the same factor)


def _dev(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=DEV)


def _f32(x):  # what the device sees
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _pixel_residual(model, M, pa, pb):
    """pixel residuals of a de-normalised model: reprojection error in image B (H), Sampson distance (F)"""
    ha, hb = np.c_[pa, np.ones(len(pa))], np.c_[pb, np.ones(len(pb))]
    if model == gr.HOMOGRAPHY:
        p = ha @ M.T
        return np.linalg.norm(p[:, :2] / p[:, 2:] - pb, axis=1)
    la, lb = ha @ M.T, hb @ M
    d = (hb * la).sum(1)
    return np.abs(d) / np.sqrt(la[:, 0] ** 2 + la[:, 1] ** 2 + lb[:, 0] ** 2 + lb[:, 1] ** 2)


def _score_bound(model, pa, pb, thr, ms):
    """f32 error bound of the sums of rho of the normalised models ms: a relative error REL_R in each row's residual r moves rho
    by |d rho / dr| REL_R r = w 2 V REL_R, plus n 2^-22 sum rho for the f32 sums; added over the models"""
    S, rho, w, V = mr.scores(model, pa, pb, thr, np.stack(ms))
    Vf = np.where(np.isfinite(V), V, 0.0)
    n = len(pa)
    return S, float((w * 2 * Vf * REL_R).sum() + n * 2.0 ** -22 * S.sum())


def _model_metric(model, Ma, Mb, truth):
    """distance of two pixel models: H corner error between them; F difference of their mean epipolar distances of the noise-free
    correspondences truth = (pa, pb0)"""
    if model == gr.HOMOGRAPHY:
        return corner_error(Ma, Mb)
    return abs(f_error(Ma, *truth) - f_error(Mb, *truth))


def _agreement(model, pa, pb, thr, seed, conf, max_iters, truth=None):
    from roma_amd.geometry import magsac
    M, mask, ok, info, score = magsac(model, _dev(pa)[None], _dev(pb)[None], thr, conf, max_iters, seed=seed)
    pa32, pb32 = _f32(pa), _f32(pb)
    ref = mr.magsac(model, pa32, pb32, thr, conf, max_iters, seed)
    ref32 = mr.magsac(model, pa32, pb32, thr, conf, max_iters, seed, f32=True)
    info, mask, M, score = info[0].cpu().numpy(), mask[0].cpu().numpy(), M[0].cpu().numpy(), score[0].cpu().numpy()
    sens = _model_metric(model, ref["M"], ref32["M"], truth)
    dist = _model_metric(model, ref["M"], M, truth)
    same = (info[1], info[2]) == (ref["best_h"], ref["best_root"])
    print(f"model {model} seed {seed}: rounds {info[0]}/{ref['rounds']} winner {tuple(info[1:3])}/{(ref['best_h'], ref['best_root'])} "
          f"score {score}/{(ref['score_min'], ref['score'])} lo {info[6]}/{ref['lo_steps']} model distance {dist:.3e} "
          f"oracle f32 sensitivity {sens:.3e} mask diffs {(mask != ref['mask']).sum()}")
    assert bool(ok[0]) and ref["ok"]
    assert info[0] == ref["rounds"], (info, ref["rounds"])  # the same early stop
    if not same:  # a different winner only where the oracle's sums of rho of the two winners lie within the f32 error bound
        m_dev = mr.minimal_model(model, pa32, pb32, seed, int(info[1]), int(info[2]))
        m_ref = mr.minimal_model(model, pa32, pb32, seed, ref["best_h"], ref["best_root"])
        assert m_dev is not None
        S, bound = _score_bound(model, pa32, pb32, thr, [m_dev, m_ref])
        print(f"  winners differ: oracle sums {S}, |difference| {abs(S[0] - S[1]):.4e}, bound {bound:.4e}")
        assert abs(S[0] - S[1]) <= bound, (S, bound)
    diff = mask != ref["mask"]
    if diff.any():  # only rows whose residual lies within REL_R of the threshold
        r = _pixel_residual(model, ref["M"], pa32[diff], pb32[diff])
        assert np.all(np.abs(r / thr - 1) < REL_R), r / thr
    assert dist <= MARGIN * sens, (dist, sens)
    assert score[1] <= score[0] and 0 <= info[6] <= mr.LO_ITERS
    return info


def test_against_reference_homography(built_lib):
    """Measured on an MI355X (corner error between the device's and the f64 oracle's final H; the bound is 10 x the oracle's
    own f32-residual sensitivity): seed 1: 3.27e-6 px, sensitivity 3.27e-6 (LO 6 / 6 steps); seed 2: 9.00e-6 px, sensitivity
    9.00e-6 (LO 7 / 10 steps); seed 3: 1.03e-6 px, sensitivity 1.03e-6 (LO 5 / 5).  Winners, rounds and masks are equal."""
    rng = np.random.default_rng(2)
    H, pa, pb, truth = _homography_scene(n=2000, outlier_frac=0.3, seed=4)
    pb = pb + 0.5 * rng.normal(size=pb.shape)
    for seed in (1, 2, 3):
        _agreement(gr.HOMOGRAPHY, pa, pb, 3.0, seed, 0.995, 2000)


def test_against_reference_fundamental(built_lib):
    K, R, t, Ft, pa, pb, truth = relief_scene(n=2000, noise_px=0.5, thr=1.0, rng_seed=3)
    pb0 = relief_scene(n=2000, noise_px=0.0, thr=1.0, rng_seed=3)[5]  # the same draws without the noise
    tr = (_f32(pa)[truth], pb0[truth])
    for seed in (1, 2, 3):
        _agreement(gr.FUNDAMENTAL, pa, pb, 1.0, seed, 0.999, 2000, tr)


def test_quality_against_device_ransac_on_local_outliers(built_lib):
    """On the scenes of tests/test_cpu_magsac.py (oracle ratios 0.038 for H, 0.061 for F): device MAGSAC++ has a median error at
    most half that of the device RANSAC + LO with the same seed and threshold."""
    from roma_amd import find_fundamental, find_homography
    for name, args, scene, fn in (("H", H_ARGS, h_local_scene, find_homography), ("F", F_ARGS, f_local_scene, find_fundamental)):
        er, em = [], []
        for s in SCENES:
            sc = scene(s)
            pa, pb = sc[1], sc[2]
            Mr, _ = fn(_dev(pa), _dev(pb), *args, seed=s, refine=True)
            Mm, _ = fn(_dev(pa), _dev(pb), *args, seed=s, refine=True, method="magsac")
            assert Mr is not None and Mm is not None
            if name == "H":
                er.append(corner_error(sc[0], Mr.cpu().numpy()))
                em.append(corner_error(sc[0], Mm.cpu().numpy()))
            else:
                er.append(f_error(Mr.cpu().numpy(), _f32(pa), sc[3]))
                em.append(f_error(Mm.cpu().numpy(), _f32(pa), sc[3]))
        ratio = float(np.median(np.array(em) / np.array(er)))
        print(f"{name}: ransac {np.round(er, 4)} magsac {np.round(em, 4)} median ratio {ratio:.3f}")
        assert ratio <= 0.5, (name, ratio)


@pytest.mark.parametrize("model", [0, 1])
def test_batch_equals_single_pairs_and_is_deterministic(built_lib, model):
    from roma_amd.geometry import magsac
    counts = [700, 350, 1000, 9, 512]
    B, N = len(counts), max(counts)
    A = np.full((B, N, 2), np.nan, dtype=np.float32)
    Bp = np.full((B, N, 2), np.nan, dtype=np.float32)
    for b, n in enumerate(counts):
        if model == 0:
            _, pa, pb, _ = _homography_scene(n=n, outlier_frac=0.3, seed=20 + b)
        else:
            _, _, _, _, pa, pb, _ = relief_scene(n=n, noise_px=0.3, thr=1.0, rng_seed=20 + b)
        A[b, :n], Bp[b, :n] = pa, pb
    seeds = torch.tensor([11, 12, 13, 14, 15], dtype=torch.int64)
    thr = 3.0 if model == 0 else 1.0
    out = magsac(model, _dev(A), _dev(Bp), thr, 0.999, 1500, seed=seeds, counts=torch.tensor(counts))
    out2 = magsac(model, _dev(A), _dev(Bp), thr, 0.999, 1500, seed=seeds, counts=torch.tensor(counts))
    assert all(torch.equal(x, y) for x, y in zip(out, out2))
    M, mask, ok, info, score = out
    assert not torch.isnan(M).any() and ok.cpu().tolist() == [True] * 5
    for b, n in enumerate(counts):
        Ms, ms, oks, infs, scs = magsac(model, _dev(A[b, :n])[None], _dev(Bp[b, :n])[None], thr, 0.999, 1500, seed=int(seeds[b]))
        assert torch.equal(Ms[0], M[b]) and torch.equal(ms[0], mask[b, :n]) and torch.equal(infs[0], info[b])
        assert torch.equal(scs[0], score[b]) and torch.equal(oks[0], ok[b])
        assert not mask[b, n:].any()


def test_degenerate_input(built_lib):
    from roma_amd import find_fundamental, find_homography
    from roma_amd.geometry import magsac
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 500, (7, 2))
    assert find_homography(_dev(pts[:3]), _dev(pts[:3] + 5), method="magsac") == (None, None)
    assert find_fundamental(_dev(pts[:6]), _dev(pts[:6] + 5), method="magsac") == (None, None)
    M, mask, ok, info, score = magsac(0, _dev(pts)[None].repeat(2, 1, 1), _dev(pts + 3)[None].repeat(2, 1, 1), 3.0, 0.99, 500,
                                      seed=1, counts=torch.tensor([3, 7]))
    assert ok.cpu().tolist() == [False, True] and not mask[0].any() and not torch.isnan(M).any()
    s = np.linspace(0, 400, 200)
    line = np.stack([s, 0.3 * s + 20], 1)
    same = np.full((200, 2), 123.0)
    for model in (0, 1):
        for lo in (0, 10):
            for a, b in ((line, 1.5 * line + 7), (same, same + 1)):
                M, mask, ok, info, score = magsac(model, _dev(a)[None], _dev(b)[None], 3.0, 0.99, 1000, seed=2, lo_iters=lo)
                assert not bool(ok[0]) and not torch.isnan(M).any() and not mask.any() and not torch.isnan(score).any()
    # exactly the minimal number of points in general position: the model fits them (with and without LO)
    H = np.array([[1.05, 0.02, 10.0], [0.01, 0.97, -4.0], [1e-4, 2e-5, 1.0]])
    q = np.c_[pts[:4], np.ones(4)] @ H.T
    fb = rng.uniform(0, 500, (7, 2))
    for refine in (False, True):
        Hp, m = find_homography(_dev(pts[:4]), _dev(q[:, :2] / q[:, 2:]), 3.0, seed=3, refine=refine, method="magsac")
        assert Hp is not None and m.all() and not torch.isnan(Hp).any()
        qa = np.c_[pts[:4], np.ones(4)] @ Hp.cpu().numpy().T
        assert np.abs(qa[:, :2] / qa[:, 2:] - q[:, :2] / q[:, 2:]).max() < 1e-2
        F, m = find_fundamental(_dev(pts), _dev(fb), 1.0, seed=3, refine=refine, method="magsac")
        assert F is not None and m.all() and not torch.isnan(F).any()
        da, db = epipolar_dist(F.cpu().numpy(), _f32(pts), _f32(fb))
        assert max(da.max(), db.max()) < 1e-2


def test_scores_never_rise_and_lo_is_bounded(built_lib):
    from roma_amd.geometry import magsac
    for model, scene, args in ((0, h_local_scene, H_ARGS), (1, f_local_scene, F_ARGS)):
        sc = [scene(s) for s in SCENES]
        A = np.stack([x[1] for x in sc])
        Bp = np.stack([x[2] for x in sc])
        seeds = torch.tensor(SCENES, dtype=torch.int64)
        for lo in (0, 3, 10):
            M, mask, ok, info, score = magsac(model, _dev(A), _dev(Bp), *args, seed=seeds, lo_iters=lo)
            info, score = info.cpu().numpy(), score.cpu().numpy()
            assert ok.all() and (score[:, 1] <= score[:, 0]).all() and (info[:, 6] <= lo).all(), (score, info)
            assert (info[:, 4] == mask.sum(1).cpu().numpy()).all()
            if lo == 0:
                assert (score[:, 1] == score[:, 0]).all() and (info[:, 4] == info[:, 3]).all()


def test_default_method_is_unchanged(built_lib):
    from roma_amd import find_fundamental, find_homography
    _, pa, pb = h_local_scene(0, n=2000)
    _, fa, fb, _ = f_local_scene(0, n=2000)
    for fn, a, b in ((find_homography, pa, pb), (find_fundamental, fa, fb)):
        x, y = _dev(a), _dev(b)
        for refine in (False, True):
            r0 = fn(x, y, 3.0, 0.999, 1000, seed=4, refine=refine)
            r1 = fn(x, y, 3.0, 0.999, 1000, seed=4, refine=refine, method="ransac")
            assert all(torch.equal(u, v) for u, v in zip(r0, r1))
            rb0 = fn(x[None], y[None], 3.0, 0.999, 1000, seed=4, refine=refine)
            rb1 = fn(x[None], y[None], 3.0, 0.999, 1000, seed=4, refine=refine, method="ransac")
            assert all(torch.equal(u, v) for u, v in zip(rb0, rb1))


def test_demo_fundamental_pipeline_with_magsac(built_lib, weights0):
    """demo_fundamental with its own estimator: match -> sample -> to_pixel_coordinates ->
    findFundamentalMat(0.2, 0.999999, 10000, USAC_MAGSAC) as find_fundamental(..., method="magsac"), with the relief scene's
    exact correspondences standing in for match() (sample does not use the weights)."""
    from accuracy_harness import synthetic_relief_pair
    from roma_amd import find_fundamental, roma_model
    sd, dsd = weights0
    model = roma_model((112, 112), True, device=DEV, weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                       upsample_res=(168, 168), max_batch=1)
    h, w = 240, 320
    d = synthetic_relief_pair(h, w, seed=3)
    warp, cert = d["gt_matches"].to(DEV), d["gt_certainty"].to(DEV)
    torch.manual_seed(0)
    matches, certainty = model.sample(warp, cert, num=5000)
    kA, kB = model.to_pixel_coordinates(matches, h, w, h, w)
    F, mask = find_fundamental(kA, kB, 0.2, 0.999999, 10000, seed=0, method="magsac")
    assert F is not None and F.is_cuda and mask.is_cuda
    T = d["T_1to2"]
    K = d["K1"]
    Fn = F.cpu().numpy()
    E = K.T @ Fn @ K
    Ki = np.linalg.inv(K)
    pa, pb = kA.cpu().double().numpy(), kB.cpu().double().numpy()
    x0, x1 = (np.c_[pa, np.ones(len(pa))] @ Ki.T)[:, :2], (np.c_[pb, np.ones(len(pb))] @ Ki.T)[:, :2]
    _, Rp, tp, _ = pg.recover_pose(E, x0, x1, mask.cpu().numpy())
    e_t, e_R = pg.compute_pose_error(np.c_[T[:, :3], T[:, 3]], Rp, tp)
    print(f"demo pipeline with MAGSAC++: e_R {float(e_R):.4f} deg, e_t {float(e_t):.4f} deg, inliers {int(mask.sum())}")
    assert e_R < 1.0 and e_t < 2.0, (e_R, e_t)
