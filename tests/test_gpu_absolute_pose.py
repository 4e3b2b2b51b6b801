"""Device absolute pose (roma_amd.estimate_absolute_pose / absolute_pose / absolute_pose_minimal / refine_absolute_pose /
lift_matches, csrc/absolute_pose.hip) against its numpy restatement tools/absolute_pose_ref.py and against exact geometry;
tails, ragged counts, determinism, the world origin.  Everything the device is compared with goes through f32 first: the
oracle gets what the device sees."""
import numpy as np
import pytest
import torch

from absolute_pose_cases import THR, ar, exact_samples, f32, relief_depth, reproj2, rot_angle_deg, scene, true_pose_error

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# |R_device - R_oracle|_F and |t_device - t_oracle| of the LM fits: the bound test_gpu_pose_refine.py holds refine_pose to
# against tools/pose_refine_ref.py (ten times the 7.2e-10 measured there; the yardstick is the step-length stop 1e-10)
LM_TOL = 7.2e-9


def _dev(x, dtype=np.float32):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def test_minimal_solver_matches_the_oracle(built_lib):
    from roma_amd import absolute_pose_minimal
    Xe, xe, Rt, tt = exact_samples(4096, seed=3)
    rng = np.random.default_rng(4)
    X = np.concatenate([Xe, rng.uniform(-2, 2, (4096, 3, 3)) + [0, 0, 5.0]])
    x = np.concatenate([xe, rng.uniform(-0.6, 0.6, (4096, 3, 2))])
    R, t, n = absolute_pose_minimal(_dev(X, np.float64), _dev(x, np.float64))
    assert tuple(R.shape) == (8192, 4, 3, 3) and tuple(t.shape) == (8192, 4, 3) and R.dtype == torch.float64 and n.dtype == torch.int32
    R, t, n = R.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()
    Rr, tr, nr = ar.p3p(X, x)
    same = n == nr
    print(f"same solution count {same.mean():.5f}, solutions {np.bincount(n, minlength=5)}")
    assert same.mean() >= 0.995, same.mean()
    d = np.array([max(np.abs(R[i, :n[i]] - Rr[i, :n[i]]).max(), np.abs(t[i, :n[i]] - tr[i, :n[i]]).max()) if n[i] else 0.0
                  for i in np.nonzero(same)[0]])
    print(f"difference to the oracle: median {np.median(d):.2e}, 99.5 % {np.percentile(d, 99.5):.2e}, worst {d.max():.2e}")
    assert (d < 1e-8).mean() >= 0.995 and np.median(d) < 1e-12, np.percentile(d, [50, 99, 100])
    for s in range(4):
        assert not R[s >= n, s].any() and not t[s >= n, s].any()
    err = true_pose_error(R[:4096], t[:4096], n[:4096], Rt, tt)
    assert (err < 1e-9).mean() >= 0.995 and (err > 1e-6).sum() == 0, (np.percentile(err, [50, 99.5]), np.sort(err)[-5:])


def _agreement(K, X, kp, seed, conf=0.9999, max_iters=1000):
    from roma_amd.absolute_pose import absolute_pose
    X, kp = f32(X), f32(kp)
    R, t, mask, ok, info = absolute_pose(_dev(X)[None], _dev(kp)[None], K, THR, conf, max_iters, seed=seed)
    ref = ar.ransac(X, kp, K, THR, conf, max_iters, seed)
    info, mask = info[0].cpu().numpy(), mask[0].cpu().numpy()
    assert bool(ok[0]) and ref["ok"] and info[4] == 1
    assert info[0] == ref["rounds"]
    assert (info[1], info[2]) == (ref["best_h"], ref["best_root"]) or info[3] == ref["best"], (info, ref)
    diff = mask != ref["mask"]
    print(f"winner {info[1:4]} oracle {ref['best_h'], ref['best_root'], ref['best']}, {diff.sum()} rows differ")
    assert diff.mean() <= 1e-3
    if (info[1], info[2]) == (ref["best_h"], ref["best_root"]):
        dR, dt = np.abs(R[0].cpu().numpy() - ref["R"]).max(), np.abs(t[0, :, 0].cpu().numpy() - ref["t"]).max()
        print(f"|dR| {dR:.2e} |dt| {dt:.2e}")
        assert dR < 1e-8 and dt < 1e-8, (dR, dt)
        # a differing row sits at the threshold: its squared reprojection error is within a relative 1e-4 of thr^2
        thr_n = THR / ((K[0, 0] + K[1, 1]) / 2)
        r2 = reproj2(ref["R"], ref["t"], X, kp, K)
        print("differing rows, r^2 / thr^2 - 1:", r2[diff] / thr_n ** 2 - 1)
        assert (np.abs(r2[diff] / thr_n ** 2 - 1) < 1e-4).all()
    return R[0], t[0], ref


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("frac", [0.3, 0.5])
def test_agreement_with_the_oracle(built_lib, seed, frac):
    K, R, t, X, kp, truth = scene(n=2000, outlier_frac=frac, noise_px=0.3)
    _agreement(K, X, kp, seed)


def test_world_origin_far_from_the_points(built_lib):
    """the scene's points moved by (1e3, -2e3, 5e2): without the centring and scaling of the 3-D rows the f32 scoring would
    work on numbers of 2e3 with a threshold of 2e-3"""
    K, R, t, X, kp, truth = scene(n=2000, outlier_frac=0.3, noise_px=0.3, shift=(1e3, -2e3, 5e2))
    Rd, td, ref = _agreement(K, X, kp, seed=1)
    # f32 rounding of coordinates of 2e3 moves a point by up to 1.2e-4, a fortieth of a pixel at depth 4: the pose is the scene's
    assert rot_angle_deg(Rd.cpu().numpy(), R) < 0.5 and np.linalg.norm(td[:, 0].cpu().numpy() - t) < 0.05 * np.linalg.norm(t)


def _ragged_batch(fill):
    """B = 6 pairs of N = 257 rows with counts (0, 3, 4, 63, 65, 257); rows beyond counts[b] hold `fill`; the first four rows of
    every pair are inliers"""
    counts = [0, 3, 4, 63, 65, 257]
    Xs, ks = np.full((6, 257, 3), fill), np.full((6, 257, 2), fill)
    for b, c in enumerate(counts):
        K, R, t, X, kp, truth = scene(n=257, outlier_frac=0.2, noise_px=0.3, rng_seed=20 + b)
        order = np.r_[np.nonzero(truth)[0][:4], np.setdiff1d(np.arange(257), np.nonzero(truth)[0][:4])]
        Xs[b, :c], ks[b, :c] = X[order][:c], kp[order][:c]
    return K, Xs, ks, counts


def _run(K, X, kp, counts, seeds, max_iters, conf=0.9999):
    """(R, t, mask, ok, info) of the RANSAC and (R, t, mask, info) of the refinement that follows it"""
    from roma_amd import refine_absolute_pose
    from roma_amd.absolute_pose import absolute_pose
    a = absolute_pose(X, kp, K, THR, conf, max_iters, seed=seeds, counts=counts)
    return a + refine_absolute_pose(a[0], a[1], X, kp, K, THR, counts=counts, valid=a[3])


@pytest.mark.parametrize("max_iters", [256, 300])  # one round and two
def test_tails_ragged_counts_and_rows_beyond_counts(built_lib, max_iters):
    from roma_amd import estimate_absolute_pose
    K, X, kp, counts = _ragged_batch(np.nan)
    seeds = torch.arange(31, 37)
    conf = 1.0  # the adaptive count never ends the sampling early, except where every row is an inlier (the pair of 4 rows)
    out = _run(K, _dev(X), _dev(kp), torch.tensor(counts), seeds, max_iters, conf)
    R, t, mask, ok, info, Rr, tr, maskr, infor = out
    assert ok.cpu().tolist() == [False, False, True, True, True, True], ok
    assert info[:, 0].cpu().tolist() == ([0, 0, 1, 1, 1, 1] if max_iters == 256 else [0, 0, 1, 2, 2, 2]), info
    assert info[:, 4].cpu().tolist() == [0, 0, 1, 1, 1, 1] and bool((infor[2:, 3] == 1).all()) and not bool(infor[:2].any())
    for x in (R[:2], t[:2], mask[:2], Rr[:2], tr[:2], maskr[:2]):
        assert not bool(x.any())
    # rows beyond counts[b] are never read: huge values in their place change nothing
    K, X2, kp2, _ = _ragged_batch(3e38)
    again = _run(K, _dev(X2), _dev(kp2), torch.tensor(counts), seeds, max_iters, conf)
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    E = estimate_absolute_pose(_dev(X), _dev(kp), K, THR, conf, max_iters, seed=seeds, counts=torch.tensor(counts))
    assert torch.equal(E[0], Rr) and torch.equal(E[1], tr) and torch.equal(E[3], ok) and torch.equal(E[2][2:], maskr[2:])
    for b, c in enumerate(counts):
        assert not bool(mask[b, c:].any()) and not bool(maskr[b, c:].any())
        if c < 4:  # no pair of fewer than four rows is sampled: nothing to compare beyond the zeros above
            continue
        one = _run(K, _dev(X[b:b + 1, :c]), _dev(kp[b:b + 1, :c]), None, int(seeds[b]), max_iters, conf)
        for x, y in zip(out, one):
            assert torch.equal(x[b:b + 1, :c] if x.dim() == 2 and x.shape[1] == 257 else x[b:b + 1], y), (b, c)
    # the single-pair form: a pose for the pairs that have one, None otherwise
    assert estimate_absolute_pose(_dev(X[1, :3]), _dev(kp[1, :3]), K, THR, seed=32) is None
    Rs, ts, ms = estimate_absolute_pose(_dev(X[5]), _dev(kp[5]), K, THR, conf, max_iters, seed=36)
    assert torch.equal(Rs, Rr[5]) and torch.equal(ts, tr[5]) and torch.equal(ms, maskr[5]) and tuple(ts.shape) == (3, 1)


def test_determinism_and_independence_of_the_batch(built_lib):
    scenes = [scene(n=700, outlier_frac=f, noise_px=0.3, rng_seed=s) for f, s in ((0.2, 1), (0.4, 2), (0.1, 3), (0.5, 4))]
    K = scenes[0][0]
    X, kp = _dev(np.stack([s[3] for s in scenes])), _dev(np.stack([s[4] for s in scenes]))
    seeds = torch.tensor([11, 12, 13, 14])
    out = _run(K, X, kp, None, seeds, 600)
    assert bool(out[3].all()) and bool((out[8][:, 0] > 0).all())
    again = _run(K, X, kp, None, seeds, 600)
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    perm = [2, 0, 3, 1]
    moved = _run(K, X[perm], kp[perm], None, seeds[perm], 600)
    assert all(torch.equal(x[perm], y) for x, y in zip(out, moved))
    for b in range(4):
        one = _run(K, X[b:b + 1], kp[b:b + 1], None, seeds[b:b + 1], 600)
        assert all(torch.equal(x[b:b + 1], y) for x, y in zip(out, one)), b


def test_refinement_matches_the_oracle(built_lib):
    from roma_amd import refine_absolute_pose
    worst = 0.0
    for seed in range(4):
        K, R, t, X, kp, truth = scene(n=2000, outlier_frac=0.3, noise_px=0.5, rng_seed=10 + seed)
        X, kp = f32(X), f32(kp)
        r = ar.ransac(X, kp, K, THR, 0.9999, 1000, seed)
        o = ar.refine(r["R"], r["t"], X, kp, K, THR)
        Rd, td, mask, info = refine_absolute_pose(_dev(r["R"], np.float64), _dev(r["t"][:, None], np.float64), _dev(X), _dev(kp), K, THR)
        assert Rd.dtype == torch.float64 and tuple(td.shape) == (3, 1) and mask.dtype == torch.bool and info.dtype == torch.int32
        Rd, td, got = Rd.cpu().numpy(), td.cpu().numpy()[:, 0], info.cpu().tolist()
        dR, dt = float(np.linalg.norm(Rd - o["R"])), float(np.linalg.norm(td - o["t"]))
        worst = max(worst, dR, dt)
        print(f"seed {seed}: |dR| {dR:.3e} |dt| {dt:.3e} info {got} oracle {o['info']} cost {o['cost0']:.6e} -> {o['cost']:.6e}")
        assert got[0] == o["info"][0] and got[0] >= 1 and got[2:] == list(o["info"][2:]), (got, o["info"])
        # rows whose error sits at the threshold may fall either way; everywhere else the mask is the oracle's
        thr_n = THR / ((K[0, 0] + K[1, 1]) / 2)
        edge = np.abs(reproj2(o["R"], o["t"], X, kp, K) / thr_n ** 2 - 1) < 1e-9
        assert np.array_equal(mask.cpu().numpy()[~edge], o["mask"][~edge])
        # the truncated cost never rises
        Xn, xn, _, c, s, tn, _ = ar.normalise(X, kp, K, THR)
        cost = lambda Rx, tx: ar.lm_ref.truncated(ar.residuals(Rx, s * (Rx @ c + tx), Xn, xn), tn)[0]  # noqa: E731
        assert cost(Rd, td) <= cost(r["R"], r["t"])
    print(f"worst difference {worst:.3e}")
    assert worst <= LM_TOL, worst


def test_refinement_leaves_what_it_cannot_fit(built_lib):
    from roma_amd import refine_absolute_pose
    K, R, t, X, kp, truth = scene(n=500, outlier_frac=0.2, noise_px=0.3)
    Rs = np.stack([R, R, R])
    ts = np.stack([t + [0.002, 0, 0], t + [0, 0, -100.0], t + [0.002, 0, 0]])[:, :, None]  # pair 1: every point behind the camera
    Xb, kb = _dev(np.stack([X] * 3)), _dev(np.stack([kp] * 3))
    Ro, to, mask, info = refine_absolute_pose(_dev(Rs, np.float64), _dev(ts, np.float64), Xb, kb, K, THR, valid=torch.tensor([True, True, False]))
    info = info.cpu().tolist()
    assert info[0][0] >= 1 and info[0][3] == 1 and bool(mask[0].any())
    # a start with no active rows comes back as it went in, and info says so: no step, one cost evaluation, no active row
    assert info[1] == [0, 1, 0, 1] and not bool(mask[1].any())
    assert np.array_equal(Ro[1].cpu().numpy(), Rs[1]) and np.array_equal(to[1].cpu().numpy(), ts[1])
    # a pair that is not valid is untouched
    assert info[2] == [0, 0, 0, 0] and not bool(mask[2].any())
    assert np.array_equal(Ro[2].cpu().numpy(), Rs[2]) and np.array_equal(to[2].cpu().numpy(), ts[2])


def _lift_case():
    """a 9 x 13 depth map with zeros, a NaN and a negative entry; matches on pixel centres, on cell borders and outside"""
    H, W = 9, 13
    rng = np.random.default_rng(5)
    depth = rng.uniform(2, 6, (H, W)).astype(np.float32)
    depth[2, 3], depth[6, 10], depth[4, 7], depth[0, 12] = 0.0, 0.0, np.nan, -1.0
    K = np.array([[11.0, 0, 6.4], [0, 12.5, 4.6], [0, 0, 1]])
    px = np.r_[np.arange(W) + 0.5, np.arange(W + 1.0), [-1.0, W + 1.0, 0.25, W - 0.25], rng.uniform(0, W, 40)]
    py = np.r_[np.arange(H) + 0.5, np.arange(H + 1.0), [-1.0, H + 1.0, 0.25, H - 0.25], rng.uniform(0, H, 40)]
    gx, gy = np.meshgrid(px, py)
    m = np.stack([2 * gx.ravel() / W - 1, 2 * gy.ravel() / H - 1, rng.uniform(-1.2, 1.2, gx.size), rng.uniform(-1.2, 1.2, gx.size)], 1)
    return m.astype(np.float32), depth, K


def test_lift_matches_against_its_restatement(built_lib):
    from roma_amd import lift_matches
    m, depth, K = _lift_case()
    pts, kb = lift_matches(_dev(m), _dev(depth), K, 480, 640)
    assert tuple(pts.shape) == (len(m), 3) and tuple(kb.shape) == (len(m), 2) and pts.dtype == torch.float32
    pr, kr = ar.lift_matches(m, depth, K, 480, 640)
    pts, kb = pts.cpu().numpy(), kb.cpu().numpy()
    nan = np.isnan(pr).any(axis=1)
    assert 0.1 < nan.mean() < 0.9
    assert np.array_equal(np.isnan(pts), np.isnan(pr)) and np.array_equal(np.isnan(pts).any(axis=1), np.isnan(pts).all(axis=1))
    assert np.array_equal(pts[~nan], pr[~nan]) and np.array_equal(kb, kr)
    # batched, another depth map and camera per pair
    d2, K2 = np.stack([depth, depth[::-1].copy()]), np.stack([K, K * [[1.5], [0.5], [1]]])
    pb, kbb = lift_matches(_dev(np.stack([m, m])), _dev(d2), K2, 100, 50)
    for b in range(2):
        p1, k1 = ar.lift_matches(m, d2[b], K2[b], 100, 50)
        assert np.array_equal(pb[b].cpu().numpy(), p1, equal_nan=True) and np.array_equal(kbb[b].cpu().numpy(), k1)


def test_localize_on_a_relief_scene(built_lib, weights0):
    """The scene's exact matches lifted with its depth map: the pose is the scene's up to what bilinear depth on the relief
    allows.  The numpy restatement on these matches (measured here, on the CPU, every run): rotation 2.5e-4 degrees, translation
    2.0e-5 at |t| = 0.44.  The device differs from it by the f32 rounding of the points only: twice that is the bound."""
    from roma_amd import roma_model
    sd, dsd = weights0
    model = roma_model((112, 112), True, device=DEV, weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                       upsample_res=(168, 168), max_batch=1)
    h, w, n = 120, 160, 1500
    K, R, t, _, _, _ = scene(n=8, h=h, w=w)
    rng = np.random.default_rng(7)
    ph = rng.uniform(0, 6, 2)
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    depth = relief_depth(xs, ys, h, w, ph).astype(np.float32)
    pa = rng.uniform([1, 1], [w - 1, h - 1], (n, 2))
    Y = np.c_[(pa[:, 0] - K[0, 2]) / K[0, 0], (pa[:, 1] - K[1, 2]) / K[1, 1], np.ones(n)] * relief_depth(pa[:, 0], pa[:, 1], h, w, ph)[:, None]
    q = Y @ R.T + t
    pb = np.stack([K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2], K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]], 1)
    m = np.c_[2 * pa[:, 0] / w - 1, 2 * pa[:, 1] / h - 1, 2 * pb[:, 0] / w - 1, 2 * pb[:, 1] / h - 1].astype(np.float32)
    pts, kb = ar.lift_matches(m, depth, K, h, w)
    Rr, tr, _ = ar.estimate_absolute_pose(pts, kb, K, THR, seed=1)
    e_R, e_t = rot_angle_deg(Rr, R), np.linalg.norm(tr[:, 0] - t)
    print(f"restatement: rotation {e_R:.5f} degrees, translation {e_t:.3e} (|t| {np.linalg.norm(t):.3f})")
    Rd, td, mask = model.localize(_dev(m), _dev(depth), K, K, h, w, reproj_thresh=THR, seed=1)
    d_R, d_t = rot_angle_deg(Rd.cpu().numpy(), R), np.linalg.norm(td[:, 0].cpu().numpy() - t)
    print(f"device: rotation {d_R:.5f} degrees, translation {d_t:.3e}, {int(mask.sum())} inliers")
    assert d_R <= 2 * e_R and d_t <= 2 * e_t and int(mask.sum()) > 0.9 * n
    Rb, tb, mb, ok = model.localize(_dev(m)[None], _dev(depth)[None], K, K, h, w, reproj_thresh=THR, seed=1)
    assert bool(ok[0]) and torch.equal(Rb[0], Rd) and torch.equal(tb[0], td) and torch.equal(mb[0], mask)
