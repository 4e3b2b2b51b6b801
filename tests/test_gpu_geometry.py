"""Device RANSAC (roma_amd.find_homography / find_fundamental, csrc/geometry.hip) against exact geometry and against its numpy
restatement tools/geometry_ref.py; batching, determinism, degenerate input, and the demo_fundamental pipeline end to end."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_geometry import _homography_scene, epipolar_dist, relief_scene

sys.path.insert(0, os.path.join(ROOT, "tools"))
import geometry_ref as gr  # noqa: E402
import pose_geometry as pg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=DEV)


def _corner_error(H, Hp, w=864, h=864):
    """HPatches metric: mean distance of the four image corners mapped by H and by Hp"""
    c = np.array([[0, 0, 1], [w, 0, 1], [0, h, 1], [w, h, 1]], dtype=np.float64)
    a, b = c @ H.T, c @ Hp.T
    return float(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=1).mean())


def _pose_errors_deg(F, K, R, t, pa, pb, mask):
    E = K.T @ F @ K
    Ki = np.linalg.inv(K)
    x0, x1 = (np.c_[pa, np.ones(len(pa))] @ Ki.T)[:, :2], (np.c_[pb, np.ones(len(pb))] @ Ki.T)[:, :2]
    _, Rp, tp, _ = pg.recover_pose(E, x0, x1, mask)
    e_t, e_R = pg.compute_pose_error(np.c_[R, t], Rp, tp)
    return float(e_R), float(e_t)


def _f32(x):  # what the device sees
    return np.asarray(x, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize("refine", [False, True])
def test_exact_on_clean_data(built_lib, refine):
    from roma_amd import find_fundamental, find_homography
    H, pa, pb, truth = _homography_scene(n=2000, outlier_frac=0.3)
    Hp, mask = find_homography(_dev(pa), _dev(pb), 3.0, seed=5, refine=refine)
    assert Hp is not None and Hp.is_cuda and Hp.dtype == torch.float64 and mask.dtype == torch.bool
    assert np.array_equal(mask.cpu().numpy(), truth)
    Hp = Hp.cpu().numpy()
    assert abs(Hp[2, 2] - 1) < 1e-15 and _corner_error(H, Hp) < 1e-2, _corner_error(H, Hp)
    K, R, t, Ft, fa, fb, ftruth = relief_scene(n=2000)
    F, fmask = find_fundamental(_dev(fa), _dev(fb), 0.2, 0.999, 2000, seed=5, refine=refine)
    assert F is not None and np.array_equal(fmask.cpu().numpy(), ftruth)
    F = F.cpu().numpy()
    assert abs(F[2, 2] - 1) < 1e-15 and abs(np.linalg.det(F)) < 1e-9 * np.linalg.norm(F) ** 3
    da, db = epipolar_dist(F, _f32(fa)[ftruth], _f32(fb)[ftruth])
    assert np.median(np.maximum(da, db)) < 1e-3, np.median(np.maximum(da, db))


def _agreement(model, pa, pb, thr, seed, conf, max_iters):
    from roma_amd.geometry import ransac
    M, mask, ok, info = ransac(model, _dev(pa)[None], _dev(pb)[None], thr, conf, max_iters, seed=seed, refine=False)
    ref = gr.ransac(model, _f32(pa), _f32(pb), thr, conf, max_iters, seed, refine=False)
    info = info[0].cpu().numpy()
    mask = mask[0].cpu().numpy()
    assert bool(ok[0]) and ref["ok"]
    assert info[0] == ref["rounds"], (info, ref["rounds"])  # the same early stop
    same = (info[1], info[2]) == (ref["best_h"], ref["best_root"])
    assert same or info[3] == ref["best_min"], (info, ref["best_h"], ref["best_root"], ref["best_min"])
    diff = mask != ref["mask"]
    assert diff.mean() <= 1e-3, diff.sum()
    if same and diff.any():  # f32 scoring against the f64 reference: only points at the threshold may differ
        qa, qb = _f32(pa)[diff], _f32(pb)[diff]
        if model == gr.HOMOGRAPHY:
            p = np.c_[qa, np.ones(len(qa))] @ ref["M"].T
            err = np.linalg.norm(p[:, :2] / p[:, 2:] - qb, axis=1)
        else:
            err = np.maximum(*epipolar_dist(ref["M"], qa, qb))
        assert np.all(np.abs(err / thr - 1) < 1e-4), err / thr
    return info


def test_against_reference_homography(built_lib):
    rng = np.random.default_rng(2)
    H, pa, pb, truth = _homography_scene(n=2000, outlier_frac=0.3, seed=4)
    pb = pb + 0.5 * rng.normal(size=pb.shape)
    for seed in (1, 2, 3):
        _agreement(gr.HOMOGRAPHY, pa, pb, 3.0, seed, 0.995, 2000)


def test_against_reference_fundamental(built_lib):
    K, R, t, Ft, pa, pb, truth = relief_scene(n=2000, noise_px=0.5, thr=1.0, rng_seed=3)
    for seed in (1, 2, 3):
        _agreement(gr.FUNDAMENTAL, pa, pb, 1.0, seed, 0.999, 2000)
    # a low-confidence run that needs several rounds stops on the same round
    info = _agreement(gr.FUNDAMENTAL, pa, pb, 1.0, 4, 0.5, 3000)
    assert info[0] >= 1


def test_noisy_homography_corner_error_and_recall(built_lib):
    from roma_amd import find_homography
    rng = np.random.default_rng(9)
    H, pa, pb, truth = _homography_scene(n=10000, outlier_frac=0.0, seed=8)
    pb = pb + 0.5 * rng.normal(size=pb.shape)
    out = rng.random(len(pa)) < 0.3
    pb[out] = rng.uniform(0, 864, (out.sum(), 2))
    truth = ~out
    Hp, mask = find_homography(_dev(pa), _dev(pb), 3.0, seed=1)
    mask = mask.cpu().numpy()
    assert _corner_error(H, Hp.cpu().numpy()) < 1.0
    assert (mask & truth).sum() / truth.sum() >= 0.98


def test_noisy_fundamental_pose_and_refinement(built_lib):
    from roma_amd.geometry import FUNDAMENTAL, ransac
    K, R, t, Ft, pa, pb, truth = relief_scene(n=10000, noise_px=0.5, thr=1.0, rng_seed=4)
    res = {}
    for refine in (False, True):
        M, mask, ok, info = ransac(FUNDAMENTAL, _dev(pa)[None], _dev(pb)[None], 1.0, 0.999, 2000, seed=3, refine=refine)
        assert bool(ok[0])
        F, m = M[0].cpu().numpy(), mask[0].cpu().numpy()
        res[refine] = int(m.sum())
        assert res[refine] == int(info[0, 4])
    # the pose bound holds for the default (refined) estimate; the best minimal sample alone is ~3 degrees off in translation
    # direction on this short baseline (tools/geometry_ref.py gives the same numbers)
    e_R, e_t = _pose_errors_deg(F, K, R, t, _f32(pa), _f32(pb), m)
    assert e_R < 1.0 and e_t < 2.0, (e_R, e_t)
    assert res[True] >= res[False], res


@pytest.mark.parametrize("model", [0, 1])
def test_batch_equals_single_pairs_and_is_deterministic(built_lib, model):
    from roma_amd.geometry import ransac
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
    M, mask, ok, info = ransac(model, _dev(A), _dev(Bp), thr, 0.999, 1500, seed=seeds, counts=torch.tensor(counts))
    M2, mask2, ok2, info2 = ransac(model, _dev(A), _dev(Bp), thr, 0.999, 1500, seed=seeds, counts=torch.tensor(counts))
    assert torch.equal(M, M2) and torch.equal(mask, mask2) and torch.equal(ok, ok2) and torch.equal(info, info2)
    assert not torch.isnan(M).any() and ok.cpu().tolist() == [True] * 5
    for b, n in enumerate(counts):
        Ms, ms, oks, infs = ransac(model, _dev(A[b, :n])[None], _dev(Bp[b, :n])[None], thr, 0.999, 1500, seed=int(seeds[b]))
        assert torch.equal(Ms[0], M[b]) and torch.equal(ms[0], mask[b, :n]) and torch.equal(infs[0], info[b])
        assert not mask[b, n:].any()


# ---- the shared pipeline (csrc/ransac.h) under every (model, scoring) it is instantiated for
FOLD_ITERS = 600                                  # three rounds of 256 hypotheses, the last cut short
FOLD_CONFIDENCE = {"H": 0.995, "F": 0.99, "E": 0.999}  # the defaults of find_homography / find_fundamental / find_essential
FOLD_SAMPLE = {"H": 4, "F": 7, "E": 5}
FOLD_ORACLE_PAIRS = (1, 3)                        # 257 and 65 rows: see the test's docstring


@functools.lru_cache(maxsize=None)
def _fold_scene(model):
    """B = 8 pairs of N = 1000 rows, NaN beyond counts = 513, 257, 256, 65, 64, 63, S, S - 1 (around the 64-row stride of the
    score and accept waves and the 256-row stride of the normalise, refit and mask workgroups, the minimum and one below it):
    the pairs of the batch tests (clean points, 30 % gross outliers; 0.3 px of noise on the relief), E's in normalised
    coordinates.  (A, B float32 [8, 1000, 2], counts, threshold, [noise-free (pa, pb0) of the true inliers per pair])"""
    S = FOLD_SAMPLE[model]
    counts = [513, 257, 256, 65, 64, 63, S, S - 1]
    A = np.full((8, 1000, 2), np.nan, dtype=np.float32)
    Bp = np.full((8, 1000, 2), np.nan, dtype=np.float32)
    thr, clean = 3.0, []
    for b, n in enumerate(counts):
        if model == "H":
            _, pa, pb, truth = _homography_scene(n=n, outlier_frac=0.3, seed=20 + b)
            pb0 = pb
        else:
            K, _, _, _, pa, pb, truth = relief_scene(n=n, noise_px=0.3, thr=1.0, rng_seed=20 + b)
            pb0 = relief_scene(n=n, noise_px=0.0, thr=1.0, rng_seed=20 + b)[5]  # the same draws without the noise
            thr = 1.0
            if model == "E":
                Ki = np.linalg.inv(K[:2, :2])
                pa, pb, pb0 = ((Ki @ (p - K[None, :2, 2]).T).T for p in (pa, pb, pb0))
                thr = 1.0 / K[0, 0]
        A[b, :n], Bp[b, :n] = pa, pb
        clean.append((_f32(pa)[truth], pb0[truth]))
    return A, Bp, counts, thr, clean


def _fold_call(model, scoring, a, b, thr, conf, seed, counts=None):
    from roma_amd import geometry as g
    if model == "E":
        return (g.essential_magsac if scoring == "magsac" else g.essential)(a, b, None, conf, thr, FOLD_ITERS, seed=seed, counts=counts)
    return (g.magsac if scoring == "magsac" else g.ransac)("HF".index(model), a, b, thr, conf, FOLD_ITERS, seed=seed, counts=counts)


@pytest.mark.parametrize("scoring", ["count", "magsac"])
@pytest.mark.parametrize("model", ["H", "F", "E"])
def test_every_model_and_scoring_on_a_ragged_batch(built_lib, model, scoring):
    """One ragged batch through each of the six instantiations of the pipeline, at confidence 1 (every round runs) and at the
    front end's default confidence (pairs stop at different rounds): two runs are bit-equal, every pair alone on its own rows
    returns the batch's bits, no mask bit lies beyond counts, the pair one row short of a sample has no model.  The pairs of
    257 and 65 rows (one row past the 256-row workgroups and the 64-row waves) then go through the agreement helper of the
    (model, scoring)'s own test file, under its rules, at the default confidence; each helper costs a run or two of a numpy
    oracle (up to a second for E), which is why it is these two pairs and not all eight.  The helpers require a model from
    device and oracle alike, which the pairs of S rows (a single sample, with gross outliers in it) need not have.
    The seeds are the first run of eight from 31, 41, ... at which the oracle's own winner on both pairs is well conditioned
    for all three models: its inlier count does not move when its sample's normalised points are perturbed by 1e-13 relative.
    At seeds 31 - 38 the 7-point winner on the 257-row pair is a sample whose last elimination pivot is 2.8e-5 and whose cubic
    has a near-triple root (Q^3 = 2.0e-30 against R^2 = 1.1e-30): under that perturbation the oracle's own count for it reads
    189, 175, 85, 189, 184, 189, so which model the sample yields is decided by the last bits of acos and cos, and the
    helpers' rule (same winner, or the same count) has nothing to hold on to."""
    import test_gpu_essential as tge
    import test_gpu_essential_magsac as tgem
    import test_gpu_magsac as tgm
    A, Bp, counts, thr, clean = _fold_scene(model)
    S = FOLD_SAMPLE[model]
    seeds = torch.arange(41, 49, dtype=torch.int64)
    dA, dB, dc = _dev(A), _dev(Bp), torch.tensor(counts)
    for conf in (1.0, FOLD_CONFIDENCE[model]):
        out = _fold_call(model, scoring, dA, dB, thr, conf, seeds, dc)
        out2 = _fold_call(model, scoring, dA, dB, thr, conf, seeds, dc)
        assert all(torch.equal(x, y) for x, y in zip(out, out2))
        M, mask, ok, info = out[:4]
        rounds = info[:, 0].cpu().tolist()
        print(f"{model} {scoring} confidence {conf}: rounds {rounds} ok {ok.cpu().tolist()}")
        assert rounds[:6] == [3] * 6 if conf == 1.0 else max(rounds) <= 3
        for b, n in enumerate(counts):
            w = max(n, S)  # the front end launches nothing for fewer than S columns: the last pair keeps S of them
            alone = _fold_call(model, scoring, dA[b:b + 1, :w], dB[b:b + 1, :w], thr, conf, int(seeds[b]), torch.tensor([n]))
            assert torch.equal(alone[0][0], M[b]) and torch.equal(alone[1][0], mask[b, :w]) and torch.equal(alone[2][0], ok[b])
            assert all(torch.equal(x[0], y[b]) for x, y in zip(alone[3:], out[3:]))  # info, and score where there is one
            assert not mask[b, n:].any()
        valid = info[:, -2] if scoring == "magsac" else info[:, -1]  # MAGSAC++ appends the LO steps
        assert valid.cpu().tolist() == [1] * 7 + [0]
        assert not bool(ok[7]) and not M[7].any() and bool(ok[:6].all())
    for b in FOLD_ORACLE_PAIRS:
        n, seed = counts[b], int(seeds[b])
        pa, pb = A[b, :n].astype(np.float64), Bp[b, :n].astype(np.float64)
        if model == "E" and scoring == "count":
            tge._agreement(pa, pb, thr, seed, conf, FOLD_ITERS)
        elif model == "E":
            pair = [o[b].cpu().numpy() for o in out]  # E, mask, ok, info, score of the default-confidence run
            pair[1] = pair[1][:n]
            tgem._check_against_oracle(pa, pb, thr, seed, pair, None, conf, FOLD_ITERS)
        elif scoring == "count":
            _agreement("HF".index(model), pa, pb, thr, seed, conf, FOLD_ITERS)
        else:
            tgm._agreement("HF".index(model), pa, pb, thr, seed, conf, FOLD_ITERS, clean[b])


def test_degenerate_input(built_lib):
    from roma_amd import find_fundamental, find_homography
    from roma_amd.geometry import ransac
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 500, (7, 2))
    assert find_homography(_dev(pts[:3]), _dev(pts[:3] + 5)) == (None, None)
    assert find_fundamental(_dev(pts[:6]), _dev(pts[:6] + 5)) == (None, None)
    # counts below the sample size in a batch: ok = False, nothing read
    M, mask, ok, _ = ransac(0, _dev(pts)[None].repeat(2, 1, 1), _dev(pts + 3)[None].repeat(2, 1, 1), 3.0, 0.99, 500, seed=1,
                            counts=torch.tensor([3, 7]))
    assert ok.cpu().tolist() == [False, True] and not mask[0].any()
    s = np.linspace(0, 400, 200)
    line = np.stack([s, 0.3 * s + 20], 1)
    same = np.full((200, 2), 123.0)
    for model in (0, 1):
        for a, b in ((line, 1.5 * line + 7), (same, same + 1)):
            M, mask, ok, _ = ransac(model, _dev(a)[None], _dev(b)[None], 3.0, 0.99, 1000, seed=2)
            assert not bool(ok[0]) and not torch.isnan(M).any() and not mask.any()
    # exactly the minimal number of points in general position: the model fits them
    H = np.array([[1.05, 0.02, 10.0], [0.01, 0.97, -4.0], [1e-4, 2e-5, 1.0]])
    q = np.c_[pts[:4], np.ones(4)] @ H.T
    Hp, m = find_homography(_dev(pts[:4]), _dev(q[:, :2] / q[:, 2:]), 3.0, seed=3)
    assert Hp is not None and m.all()
    qa = np.c_[pts[:4], np.ones(4)] @ Hp.cpu().numpy().T
    assert np.abs(qa[:, :2] / qa[:, 2:] - q[:, :2] / q[:, 2:]).max() < 1e-2
    fb = rng.uniform(0, 500, (7, 2))
    F, m = find_fundamental(_dev(pts), _dev(fb), 1.0, seed=3)
    assert F is not None and m.all()
    da, db = epipolar_dist(F.cpu().numpy(), _f32(pts), _f32(fb))
    assert max(da.max(), db.max()) < 1e-2
    with pytest.raises(Exception, match="no CPU fallback"):
        find_fundamental(torch.zeros(10, 2), torch.zeros(10, 2))


def test_demo_fundamental_pipeline_on_device(built_lib, weights0):
    """demo_fundamental: match -> sample -> to_pixel_coordinates -> findFundamentalMat(0.2, 0.999999, 10000), with the relief
    scene's exact correspondences standing in for match() (sample does not use the weights)."""
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
    F, mask = find_fundamental(kA, kB, ransac_reproj_threshold=0.2, confidence=0.999999, max_iters=10000, seed=0)
    assert F is not None and F.is_cuda and mask.is_cuda and kA.is_cuda
    T = d["T_1to2"]
    e_R, e_t = _pose_errors_deg(F.cpu().numpy(), d["K1"], T[:, :3], T[:, 3], kA.cpu().double().numpy(), kB.cpu().double().numpy(),
                                mask.cpu().numpy())
    assert e_R < 1.0 and e_t < 2.0, (e_R, e_t)
