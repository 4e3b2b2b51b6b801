"""Device essential matrix and relative pose (roma_amd.find_essential / recover_pose / estimate_pose / essential_minimal,
csrc/essential.hip) against exact geometry, against its numpy restatement tools/essential_ref.py and against the host pose
path tools/pose_geometry.py; batching, determinism, ragged and degenerate input."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_essential import exact_samples, true_root_error
from test_cpu_geometry import relief_scene

sys.path.insert(0, os.path.join(ROOT, "tools"))
import essential_ref as er  # noqa: E402
import pose_geometry as pg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(x, dtype=np.float32):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _f32(x):  # what the device sees
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _normalised(pa, pb, K):
    Ki = np.linalg.inv(K[:2, :2])
    return _f32((Ki @ (pa - K[None, :2, 2]).T).T), _f32((Ki @ (pb - K[None, :2, 2]).T).T)


def test_minimal_solver_matches_the_oracle(built_lib):
    from roma_amd import essential_minimal
    x0e, x1e, Et = exact_samples(2048, seed=3)
    rng = np.random.default_rng(4)
    x0 = np.concatenate([x0e, rng.uniform(-1, 1, (2048, 5, 2))])
    x1 = np.concatenate([x1e, rng.uniform(-1, 1, (2048, 5, 2))])
    E, n = essential_minimal(_dev(x0, np.float64), _dev(x1, np.float64))
    E, n = E.cpu().numpy(), n.cpu().numpy()
    Er, nr = er.five_point(x0, x1)
    same = n == nr
    assert same.mean() >= 0.995, same.mean()
    d = np.array([np.linalg.norm(E[i, :n[i]] - Er[i, :n[i]], axis=(1, 2)).max() if n[i] else 0.0 for i in np.nonzero(same)[0]])
    assert (d < 1e-8).mean() >= 0.995 and np.median(d) < 1e-12, np.percentile(d, [50, 99, 100])
    err = true_root_error(E[:2048], n[:2048], Et)
    # the true E to 1e-9 on >= 99.5 % of exact samples; a miss beyond 1e-6 is a sample whose Sturm chain loses a root
    # (tools/essential_ref.py): 1 of these 2048, 4 of 4000 - at most 3 allowed here
    assert (err < 1e-9).mean() >= 0.995 and (err > 1e-6).sum() <= 3, (np.percentile(err, [50, 99.5]), np.sort(err)[-5:])


def test_exact_on_clean_data(built_lib):
    from roma_amd import estimate_pose, find_essential
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, outlier_frac=0.3)
    x0, x1 = _normalised(pa, pb, K)
    # seed 1: at some seeds a model through all inliers and one outlier wins on this near-planar relief (relief_scene)
    E, mask = find_essential(_dev(x0), _dev(x1), None, 0.999, 0.5 / K[0, 0], 1000, seed=1)
    assert E is not None and E.dtype == torch.float64 and mask.dtype == torch.bool
    assert np.array_equal(mask.cpu().numpy(), truth)
    E = E.cpu().numpy()
    assert abs(np.linalg.norm(E) - 1) < 1e-12 and E.flat[np.argmax(np.abs(E))] > 0
    Rp, tp, m = estimate_pose(_dev(pa), _dev(pb), K, K, 0.5 / K[0, 0], seed=1)
    assert tuple(tp.shape) == (3, 1)
    # against the pose of the scene's exact E: the scene's R is stored in f32, and arccos of its trace alone is 0.01 degrees off
    _, R0, t0, _ = pg.recover_pose(K.T @ F @ K, x0, x1, truth)
    e_R, e_t = pg.angle_error_mat(Rp.cpu().numpy(), R0), pg.angle_error_vec(tp.cpu().numpy()[:, 0], t0[:, 0])
    assert e_t < 1e-3 and e_R < 1e-3, (e_t, e_R)
    assert np.array_equal(m.cpu().numpy(), truth)


def _agreement(x0, x1, thr, seed, prob=0.99999, max_iters=1000):
    from roma_amd.geometry import essential
    E, mask, ok, info = essential(_dev(x0)[None], _dev(x1)[None], None, prob, thr, max_iters, seed=seed)
    ref = er.ransac(x0, x1, thr, prob, max_iters, seed)
    info, mask = info[0].cpu().numpy(), mask[0].cpu().numpy()
    assert bool(ok[0]) and ref["ok"] and info[4] == 1
    assert info[0] == ref["rounds"]
    assert (info[1], info[2]) == (ref["best_h"], ref["best_root"]) or info[3] == ref["best"], (info, ref)
    diff = mask != ref["mask"]
    assert diff.mean() <= 1e-3
    if (info[1], info[2]) == (ref["best_h"], ref["best_root"]):
        assert np.abs(E[0].cpu().numpy() - ref["E"]).max() < 1e-8
        # a differing row sits at the threshold: its Sampson error is within a relative 1e-4 of thr^2
        e = ref["E"]
        h0, h1 = np.c_[x0, np.ones(len(x0))], np.c_[x1, np.ones(len(x1))]
        l, k = h0 @ e.T, h1 @ e
        s = (h1 * l).sum(1) ** 2 / (l[:, 0] ** 2 + l[:, 1] ** 2 + k[:, 0] ** 2 + k[:, 1] ** 2)
        assert (np.abs(s[diff] / thr ** 2 - 1) < 1e-4).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("frac", [0.3, 0.5])
def test_agreement_with_reference(built_lib, seed, frac):
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, outlier_frac=frac, noise_px=0.3)
    x0, x1 = _normalised(pa, pb, K)
    _agreement(x0, x1, 0.5 / K[0, 0], seed)


def test_recover_pose_on_a_host_E(built_lib):
    from roma_amd import recover_pose
    K, R, t, F, pa, pb, truth = relief_scene(n=1500, outlier_frac=0.0, noise_px=0.5)
    x0, x1 = _normalised(pa, pb, K)
    E = K.T @ F @ K  # not exactly essential after the rounding of K^-T F K^-1 and back: the SVD takes it as it is
    mask = np.random.default_rng(0).random(len(x0)) < 0.8
    n, Rp, tp, good = recover_pose(_dev(E, np.float64), _dev(x0), _dev(x1), _dev(mask, np.bool_))
    n2, R2, t2, good2 = pg.recover_pose(E, x0, x1, mask)
    assert np.abs(Rp.cpu().numpy() - R2).max() < 1e-9 and np.abs(tp.cpu().numpy() - t2).max() < 1e-9
    # the device triangulates with the point on the ray of camera 0, pose_geometry by the 4 x 4 DLT: a row may differ only
    # where its depth is near 0 or beyond 1 / EPS (no parallax)
    z0, z1 = pg._triangulate_depths(R2, t2[:, 0], x0, x1)
    eps = 1e-6
    edge = (np.abs(z0) < eps) | (np.abs(z1) < eps) | (np.abs(z0) > 1 / eps) | (np.abs(z1) > 1 / eps)
    g = good.cpu().numpy()
    assert not ((g != good2) & ~edge).any()
    assert abs(n - n2) <= int(edge.sum()) and n == int(g.sum()) and not g[~mask].any()


def test_batch_equals_single_pairs_and_is_deterministic(built_lib):
    from roma_amd import find_essential
    scenes = [relief_scene(n=1200, outlier_frac=f, rng_seed=s) for f, s in ((0.2, 1), (0.4, 2), (0.1, 3))]
    xs = [_normalised(sc[4], sc[5], sc[0]) for sc in scenes]
    counts = [1200, 900, 600]
    a = np.full((3, 1200, 2), np.nan)
    b = np.full((3, 1200, 2), np.nan)
    for i, (x0, x1) in enumerate(xs):
        a[i, :counts[i]], b[i, :counts[i]] = x0[:counts[i]], x1[:counts[i]]
    thr = 0.5 / scenes[0][0][0, 0]
    seeds = torch.tensor([11, 12, 13])
    E, mask, ok = find_essential(_dev(a), _dev(b), None, 0.999, thr, 1000, seed=seeds, counts=torch.tensor(counts))
    E2, mask2, ok2 = find_essential(_dev(a), _dev(b), None, 0.999, thr, 1000, seed=seeds, counts=torch.tensor(counts))
    assert torch.equal(E, E2) and torch.equal(mask, mask2) and torch.equal(ok, ok2) and bool(ok.all())
    for i in range(3):
        Ei, mi = find_essential(_dev(a[i, :counts[i]]), _dev(b[i, :counts[i]]), None, 0.999, thr, 1000, seed=11 + i)
        assert torch.equal(Ei, E[i]) and torch.equal(mi, mask[i, :counts[i]]) and not bool(mask[i, counts[i]:].any())


def test_degenerate_input_gives_no_model(built_lib):
    from roma_amd import estimate_pose, find_essential
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.5, 0.5, (6, 300, 2))
    y = x + 0.01
    x[0, 4:], y[0, 4:] = np.nan, np.nan   # fewer than 5 finite rows
    x[1], y[1] = np.nan, np.nan           # all NaN
    x[2], y[2] = 0.25, -0.1               # one repeated point
    y[3] = x[3]                           # zero translation
    E, mask, ok = find_essential(_dev(x), _dev(y), None, 0.999, 1e-3, 1000, seed=1, counts=torch.tensor([300, 300, 300, 300, 4, 0]))
    ok = ok.cpu().numpy()
    assert not ok[[0, 1, 2, 4, 5]].any()
    K = np.eye(3)
    # every degenerate pair, zero translation included (no parallax: no point passes the cheirality test), has no pose
    R, t, m, ok = estimate_pose(_dev(x), _dev(y), K, K, 1e-3, seed=1, counts=torch.tensor([300, 300, 300, 300, 4, 0]))
    assert not ok.cpu().numpy().any() and not m.cpu().numpy().any()
    assert estimate_pose(_dev(x[0, :4]), _dev(y[0, :4]), K, K, 1e-3) is None


def test_estimate_pose_uncalibrated_matches_host_path(built_lib):
    from roma_amd import estimate_pose_uncalibrated, find_fundamental
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, outlier_frac=0.3)
    Rp, tp, m = estimate_pose_uncalibrated(_dev(pa), _dev(pb), K, K, 0.5, seed=2)
    Fd, fmask = find_fundamental(_dev(pa), _dev(pb), 0.5, 0.99999, 10000, seed=2)
    x0, x1 = _normalised(pa, pb, K)
    _, R2, t2, _ = pg.recover_pose(K.T @ Fd.cpu().numpy() @ K, x0, x1, fmask.cpu().numpy())
    assert pg.angle_error_mat(Rp.cpu().numpy(), R2) < 0.1
    assert pg.angle_error_vec(tp.cpu().numpy()[:, 0], t2[:, 0]) < 0.1


class _Perfect:
    """the pose benchmark's stand-in matcher: exact correspondences of a synthetic relief pair, the oracle's `sample`, the
    reference's coordinate convention (as in test_cpu_oracle.test_pose_benchmark_loop_on_synthetic_two_view_scenes)"""

    def __init__(self, pair, device):
        self.pair, self.device = pair, device

    def match(self, a, b):
        return self.pair["gt_matches"], self.pair["gt_certainty"]

    def sample(self, m, c, num):
        from oracle import roma_oracle as O
        s, cert = O.sample(m, c, num=num, generator=torch.Generator().manual_seed(5))
        return s.to(self.device), cert

    @staticmethod
    def to_pixel_coordinates(coords, H_A, W_A, H_B, W_B):
        kA, kB = coords[..., :2], coords[..., 2:]
        return (torch.stack((W_A / 2 * (kA[..., 0] + 1), H_A / 2 * (kA[..., 1] + 1)), dim=-1),
                torch.stack((W_B / 2 * (kB[..., 0] + 1), H_B / 2 * (kB[..., 1] + 1)), dim=-1))


def test_pose_benchmark_on_device_matches_host_path(built_lib):
    import accuracy_harness as AH
    dev, host = [], []
    for seed in (0, 1):
        pair = AH.synthetic_relief_pair(120, 160, seed=seed)
        dev.append(AH.pose_benchmark(_Perfect(pair, DEV), [pair], seed=seed, num=1500, repeats=2, pose="device")["auc_5"])
        host.append(AH.pose_benchmark(_Perfect(pair, "cpu"), [pair], seed=seed, num=1500, repeats=2)["auc_5"])
    assert np.mean(dev) >= 0.95 and abs(np.mean(dev) - np.mean(host)) <= 0.02, (dev, host)


def test_pose_pipeline_through_the_matcher(built_lib, weights0):
    """match -> sample -> to_pixel_coordinates -> estimate_pose in batch form, with the relief scene's exact correspondences
    standing in for match() (sample does not use the weights)."""
    from accuracy_harness import synthetic_relief_pair
    from roma_amd import estimate_pose, roma_model
    sd, dsd = weights0
    model = roma_model((112, 112), True, device=DEV, weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                       upsample_res=(168, 168), max_batch=1)
    h, w = 240, 320
    ka, kb, Ts = [], [], []
    for seed in (3, 4):
        d = synthetic_relief_pair(h, w, seed=seed)
        torch.manual_seed(seed)
        matches, _ = model.sample(d["gt_matches"].to(DEV), d["gt_certainty"].to(DEV), num=3000)
        kA, kB = model.to_pixel_coordinates(matches, h, w, h, w)
        ka.append(kA)
        kb.append(kB)
        Ts.append(d["T_1to2"])
    K = d["K1"]
    R, t, mask, ok = estimate_pose(torch.stack(ka), torch.stack(kb), K, K, 0.5 / K[0, 0], seed=torch.tensor([1, 2]))
    assert R.is_cuda and bool(ok.all())
    for i, T in enumerate(Ts):
        e_t, e_R = pg.compute_pose_error(np.asarray(T), R[i].cpu().numpy(), t[i].cpu().numpy())
        assert e_t < 2.0 and e_R < 1.0, (e_t, e_R)


def test_camera_matrix_is_applied_like_opencv(built_lib):
    from roma_amd import recover_pose
    from roma_amd.geometry import essential
    K, R, t, F, pa, pb, truth = relief_scene(n=2000, outlier_frac=0.3, noise_px=0.3)
    K = K.copy()
    K[1, 1] *= 1.05  # fx != fy: the threshold scale (fx + fy) / 2 and the per-axis normalisation both show
    thr = 0.5
    E, mask, ok, info = essential(_dev(pa)[None], _dev(pb)[None], K, 0.99999, thr, 1000, seed=2)
    ref = er.ransac(_f32(pa), _f32(pb), thr, 0.99999, 1000, 2, K=K)
    info, mask = info[0].cpu().numpy(), mask[0].cpu().numpy()
    assert bool(ok[0]) and ref["ok"] and info[0] == ref["rounds"]
    assert (info[1], info[2]) == (ref["best_h"], ref["best_root"]), (info, ref)
    assert np.abs(E[0].cpu().numpy() - ref["E"]).max() < 1e-8 and (mask != ref["mask"]).mean() <= 1e-3
    n, Rp, tp, good = recover_pose(E[0], _dev(pa), _dev(pb), mask, camera_matrix=K)
    x0 = np.stack([(_f32(pa)[:, 0] - K[0, 2]) / K[0, 0], (_f32(pa)[:, 1] - K[1, 2]) / K[1, 1]], 1)
    x1 = np.stack([(_f32(pb)[:, 0] - K[0, 2]) / K[0, 0], (_f32(pb)[:, 1] - K[1, 2]) / K[1, 1]], 1)
    n2, R2, t2, good2 = er.recover_pose(E[0].cpu().numpy(), x0, x1, mask)
    assert n == n2 and np.array_equal(good.cpu().numpy(), good2)
    assert np.abs(Rp.cpu().numpy() - R2).max() < 1e-9 and np.abs(tp.cpu().numpy() - t2).max() < 1e-9


def test_batched_pose_does_not_synchronise(built_lib):
    from roma_amd import estimate_pose, estimate_pose_uncalibrated
    K, R, t, F, pa, pb, truth = relief_scene(n=1000, outlier_frac=0.3)
    a, b = _dev(np.stack([pa, pa])), _dev(np.stack([pb, pb]))
    Kd = torch.as_tensor(K, device=DEV)
    seeds = torch.tensor([1, 2], device=DEV)
    counts = torch.tensor([1000, 800], device=DEV, dtype=torch.int32)
    estimate_pose(a, b, Kd, Kd, 0.5 / K[0, 0], seed=seeds, counts=counts)  # warm-up: library load, workspace allocator
    estimate_pose_uncalibrated(a, b, Kd, Kd, 0.5, seed=seeds, counts=counts)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        R1, t1, m1, ok1 = estimate_pose(a, b, Kd, Kd, 0.5 / K[0, 0], seed=seeds, counts=counts)
        R2, t2, m2, ok2 = estimate_pose_uncalibrated(a, b, Kd, Kd, 0.5, seed=seeds, counts=counts)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(ok1.all()) and bool(ok2.all()) and tuple(t1.shape) == (2, 3, 1)
