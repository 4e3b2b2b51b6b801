"""Device pose refinement (roma_amd.refine_pose, estimate_pose(..., refine=True); csrc/pose_refine.hip) against its numpy
restatement tools/pose_refine_ref.py and against exact geometry; batching, determinism, ragged and invalid pairs, no host
synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_geometry import relief_scene
from test_cpu_pose_refine import NOISY_CASES, NOISY_SEEDS, clean_scene, noisy_case, pose_error, starts

sys.path.insert(0, os.path.join(ROOT, "tools"))
import essential_ref as er  # noqa: E402
import pose_geometry as pg  # noqa: E402
import pose_refine_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EYE = np.eye(3)

# |R_device - R_oracle|_F and |t_device - t_oracle| over the 30 clean and 24 noisy fits below.  The two sides differ in the
# order of their sums and in their sin / cos / sqrt, so this is a rounding bound: ten times the worst difference measured on an
# MI355X (MEASURED), headroom for another compiler's choices.  The yardstick is the step-length stop 1e-10: a last step taken by
# one side only leaves a few times that; orders of magnitude more would mean an accept / reject decision went the other way.
MEASURED = 7.2e-10  # noisy 0.3 px / 30 % / seed 3: the device takes a fourth step of that length, the oracle stops after three
TOL = 10 * MEASURED


def _dev(x, dtype=np.float32):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _refine_normalised(R, t, x0, x1, thr, **kw):
    """refine_pose on normalised points: identity cameras"""
    from roma_amd import refine_pose
    return refine_pose(_dev(R, np.float64), _dev(np.reshape(t, (-1, 3, 1)) if np.ndim(R) == 3 else np.reshape(t, (3, 1)), np.float64),
                       _dev(x0), _dev(x1), EYE, EYE, thr, **kw)


def _fits():
    """(name, start R, start t, x0, x1, thr) of the clean starts (0.01 degrees off) and the 24 noisy RANSAC poses"""
    out = []
    for frac in (0.0, 0.3, 0.5):
        x0, x1, thr, R0, t0, truth = clean_scene(frac)
        out += [(f"clean {frac} {i}", Rs, ts, x0, x1, thr) for i, (Rs, ts) in enumerate(starts(R0, t0, 0.01))]
    for noise, frac in NOISY_CASES:
        K, T, pa, pb, thr = noisy_case(noise, frac)
        x0, x1 = pr.normalise(pa, pb, K, K)
        for seed in NOISY_SEEDS:
            R, t, _ = er.estimate_pose(pa, pb, K, K, thr, 0.99999, 1000, seed)
            out.append((f"noisy {noise} {frac} {seed}", R, t[:, 0], x0, x1, thr))
    return out


def test_device_matches_the_oracle(built_lib):
    worst = 0.0
    for name, Rs, ts, x0, x1, thr in _fits():
        o = pr.refine(Rs, ts, x0, x1, thr)
        R, t, mask, info = _refine_normalised(Rs, ts, x0, x1, thr)
        assert R.dtype == torch.float64 and tuple(t.shape) == (3, 1) and mask.dtype == torch.bool and info.dtype == torch.int32
        dR = float(np.linalg.norm(R.cpu().numpy() - o["R"]))
        dt = float(np.linalg.norm(t.cpu().numpy()[:, 0] - o["t"]))
        worst = max(worst, dR, dt)
        print(f"{name}: |dR| {dR:.3e} |dt| {dt:.3e} info {info.cpu().tolist()} oracle {o['info']}")
        # rows whose error sits at the threshold may fall either way; the oracle shows that these cases have none
        r2 = pr.residuals(o["R"], o["t"], x0, x1) ** 2
        edge = np.abs(r2 - thr * thr) < 1e-9 * thr * thr
        assert edge.sum() == 0
        assert np.array_equal(mask.cpu().numpy(), o["mask"]), name
        # a last step at the step-length stop may be taken by one side only; the active rows and the flag are the same
        got = info.cpu().tolist()
        assert abs(got[0] - o["info"][0]) <= 1 and got[2:] == list(o["info"][2:]), (name, got, o["info"])
    print(f"worst difference {worst:.3e}")
    assert worst <= TOL, worst


@pytest.mark.parametrize("frac", [0.0, 0.3, 0.5])
def test_exact_convergence_on_clean_data(built_lib, frac):
    x0, x1, thr, R0, t0, truth = clean_scene(frac)
    ss = starts(R0, t0, 0.01)
    R, t, mask, info = _refine_normalised(np.stack([s[0] for s in ss]), np.stack([s[1] for s in ss]), np.stack([x0] * 10),
                                          np.stack([x1] * 10), thr)
    R, t, mask, info = R.cpu().numpy(), t.cpu().numpy(), mask.cpu().numpy(), info.cpu().numpy()
    for i in range(10):
        e = pose_error(R[i], t[i, :, 0], R0, t0)
        print(f"outliers {frac} start {i}: {e:.2e} degrees, info {info[i].tolist()}")
        assert e < 1e-3 and 1 <= info[i, 0] <= 6 and info[i, 3] == 1
        assert np.array_equal(mask[i], truth) and info[i, 2] == truth.sum()


@pytest.mark.parametrize("frac,limit", [(0.0, 1), (0.3, 5)])
def test_degenerate_active_sets_return_the_input(built_lib, frac, limit):
    x0, x1, thr, R0, t0, truth = clean_scene(frac)
    chosen = [(Rs, ts) for Rs, ts in starts(R0, t0, 1.0) if pr.cost(Rs, ts, x0, x1, thr)[1] < limit]
    assert len(chosen) >= 5
    for Rs, ts in chosen:
        R, t, mask, info = _refine_normalised(Rs, ts, x0, x1, thr)
        assert np.array_equal(R.cpu().numpy(), Rs) and np.array_equal(t.cpu().numpy()[:, 0], ts)
        assert info.cpu().tolist() == [0, 1, pr.cost(Rs, ts, x0, x1, thr)[1], 1]


def _noisy_batch(noise, frac):
    K, T, pa, pb, thr = noisy_case(noise, frac)
    B = len(NOISY_SEEDS)
    return K, T, pa, pb, thr, _dev(np.stack([pa] * B)), _dev(np.stack([pb] * B)), torch.tensor(NOISY_SEEDS)


def test_estimate_pose_with_refinement_improves_the_noisy_cases(built_lib):
    from roma_amd import estimate_pose
    before, after = [], []
    for noise, frac in NOISY_CASES:
        K, T, pa, pb, thr, a, b, seeds = _noisy_batch(noise, frac)
        x0, x1 = pr.normalise(pa, pb, K, K)
        R0, t0, m0, ok0 = estimate_pose(a, b, K, K, thr, 0.99999, 1000, seed=seeds)
        R1, t1, m1, ok1 = estimate_pose(a, b, K, K, thr, 0.99999, 1000, seed=seeds, refine=True)
        assert bool(ok0.all()) and torch.equal(ok0, ok1)
        for i in range(len(NOISY_SEEDS)):
            Ra, ta, Rb, tb = R0[i].cpu().numpy(), t0[i].cpu().numpy(), R1[i].cpu().numpy(), t1[i].cpu().numpy()
            c0, c1 = pr.cost(Ra, ta[:, 0], x0, x1, thr)[0], pr.cost(Rb, tb[:, 0], x0, x1, thr)[0]
            before.append(max(pg.compute_pose_error(T, Ra, ta)))
            after.append(max(pg.compute_pose_error(T, Rb, tb)))
            print(f"noise {noise} outliers {frac} seed {NOISY_SEEDS[i]}: {before[-1]:.3f} -> {after[-1]:.3f} degrees, cost {c0:.6e} -> {c1:.6e}")
            assert c1 <= c0
            r = pr.residuals(Rb, tb[:, 0], x0, x1)
            assert np.array_equal(m1[i].cpu().numpy(), pr.active(r, thr) & er.cheirality(Rb, tb[:, 0], x0, x1, 1e9))
    before, after = np.array(before), np.array(after)
    print(f"lower in {(after < before).sum()} of {len(after)}, median {np.median(before):.3f} -> {np.median(after):.3f}")
    assert (after < before).sum() >= 20 and np.median(after) < np.median(before)


def test_batch_equals_single_pairs_ragged_counts_and_determinism(built_lib):
    from roma_amd import estimate_pose, refine_pose
    K, T, pa, pb, thr = noisy_case(0.3, 0.3)
    n = len(pa)
    counts = [n, n - 100, n - 300, 1500, 1000, 700, 4, n]
    a = np.full((8, n, 2), np.nan)
    b = np.full((8, n, 2), np.nan)
    for i, c in enumerate(counts):
        a[i, :c], b[i, :c] = pa[:c], pb[:c]
    seeds = torch.arange(8) + 1
    cd = torch.tensor(counts)
    R0, t0, m0, ok0 = estimate_pose(_dev(a), _dev(b), K, K, thr, seed=seeds, counts=cd)
    assert ok0.cpu().tolist() == [True] * 6 + [False, True]
    valid = ok0.clone()
    valid[7] = False
    out = refine_pose(R0, t0, _dev(a), _dev(b), K, K, thr, counts=cd, valid=valid)
    again = refine_pose(R0, t0, _dev(a), _dev(b), K, K, thr, counts=cd, valid=valid)
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    R, t, mask, info = out
    assert bool((info[:6, 0] > 0).all()) and info[:, 3].cpu().tolist() == [1] * 6 + [0, 0]
    for i in range(8):
        c = counts[i]
        assert not bool(mask[i, c:].any())
        if i >= 6:  # fewer than 5 rows / not valid: untouched
            assert torch.equal(R[i], R0[i]) and torch.equal(t[i], t0[i]) and not bool(mask[i].any())
            assert info[i].cpu().tolist() == [0, 0, 0, 0]
            continue
        Ri, ti, mi, ii = refine_pose(R0[i], t0[i], _dev(a[i, :c]), _dev(b[i, :c]), K, K, thr)
        assert torch.equal(Ri, R[i]) and torch.equal(ti, t[i]) and torch.equal(mi, mask[i, :c]) and torch.equal(ii, info[i])
    # estimate_pose(refine=True) is the same composition; ok is unchanged and the pairs without a pose keep their outputs
    R2, t2, m2, ok2 = estimate_pose(_dev(a), _dev(b), K, K, thr, seed=seeds, counts=cd, refine=True)
    assert torch.equal(ok2, ok0) and torch.equal(R2[:6], R[:6]) and torch.equal(t2[:6], t[:6]) and torch.equal(m2[:6], mask[:6])
    assert torch.equal(R2[6], R0[6]) and torch.equal(t2[6], t0[6]) and torch.equal(m2[6], m0[6])
    assert estimate_pose(_dev(a[6, :4]), _dev(b[6, :4]), K, K, thr, refine=True) is None


def test_counts_around_a_wave_the_workgroup_and_the_minimum(built_lib):
    """one batch whose counts leave threads and whole waves of the workgroup without rows, put one row past a wave (64) and
    past the workgroup (512), and end at MIN_ROWS and one below it; exact data, a start 0.01 degrees off"""
    x0, x1, thr, R0, t0, truth = clean_scene(0.0)
    Rs, ts = starts(R0, t0, 0.01)[0]
    n, counts = 1000, [513, 512, 511, 65, 64, 63, pr.MIN_ROWS, pr.MIN_ROWS - 1]
    a = np.full((8, n, 2), np.nan)
    b = np.full((8, n, 2), np.nan)
    for i, c in enumerate(counts):
        a[i, :c], b[i, :c] = x0[:c], x1[:c]
    cd = torch.tensor(counts)
    out = _refine_normalised(np.stack([Rs] * 8), np.stack([ts] * 8), a, b, thr, counts=cd)
    again = _refine_normalised(np.stack([Rs] * 8), np.stack([ts] * 8), a, b, thr, counts=cd)
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    R, t, mask, info = out
    for i, c in enumerate(counts):
        Ri, ti, mi, ii = _refine_normalised(Rs, ts, x0[:c], x1[:c], thr)
        assert torch.equal(Ri, R[i]) and torch.equal(ti, t[i]) and torch.equal(mi, mask[i, :c]) and torch.equal(ii, info[i]), c
        assert not bool(mask[i, c:].any())
        Rd, td, got = R[i].cpu().numpy(), t[i].cpu().numpy()[:, 0], info[i].cpu().tolist()
        print(f"count {c}: info {got}")
        if c >= 63:
            o = pr.refine(Rs, ts, x0[:c], x1[:c], thr)
            r2 = pr.residuals(o["R"], o["t"], x0[:c], x1[:c]) ** 2
            assert o["info"][0] >= 1 and (np.abs(r2 - thr * thr) < 1e-9 * thr * thr).sum() == 0
            dR, dt = float(np.linalg.norm(Rd - o["R"])), float(np.linalg.norm(td - o["t"]))
            print(f"count {c}: |dR| {dR:.3e} |dt| {dt:.3e} oracle {o['info']}")
            assert dR <= TOL and dt <= TOL, (c, dR, dt)
            assert np.array_equal(mask[i, :c].cpu().numpy(), o["mask"]) and got[2:] == list(o["info"][2:]), (c, got, o["info"])
        elif c == pr.MIN_ROWS:
            assert got[3] == 1 and pr.cost(Rd, td, x0[:c], x1[:c], thr)[0] <= pr.cost(Rs, ts, x0[:c], x1[:c], thr)[0]
        else:  # fewer rows than parameters: untouched
            assert np.array_equal(Rd, Rs) and np.array_equal(td, ts) and got == [0, 0, 0, 0] and not bool(mask[i].any())


def test_default_is_the_unrefined_path(built_lib):
    from roma_amd import estimate_pose, estimate_pose_uncalibrated
    K, T, pa, pb, thr, a, b, seeds = _noisy_batch(0.3, 0.5)
    for fn, th in ((estimate_pose, thr), (estimate_pose_uncalibrated, thr * K[0, 0])):
        plain = fn(a, b, K, K, th, seed=seeds)
        off = fn(a, b, K, K, th, seed=seeds, refine=False)
        assert all(torch.equal(x, y) for x, y in zip(plain, off))


def test_uncalibrated_refinement_scales_the_threshold(built_lib):
    from roma_amd import estimate_pose_uncalibrated, refine_pose
    K, T, pa, pb, thr, a, b, seeds = _noisy_batch(0.3, 0.3)
    K1 = K.copy()
    K1[0, 0] *= 1.1
    px = 1.0
    R0, t0, m0, ok0 = estimate_pose_uncalibrated(a, b, K, K1, px, seed=seeds)
    R1, t1, m1, ok1 = estimate_pose_uncalibrated(a, b, K, K1, px, seed=seeds, refine=True)
    focal = (K[0, 0] + K[1, 1] + K1[0, 0] + K1[1, 1]) / 4
    R2, t2, m2, info = refine_pose(R0, t0, a, b, K, K1, px / focal, valid=ok0)
    assert bool(ok0.all()) and torch.equal(ok0, ok1) and bool((info[:, 3] == 1).all()) and bool((info[:, 0] > 0).any())
    assert torch.equal(R1, R2) and torch.equal(t1, t2) and torch.equal(m1, m2)


def test_batched_refinement_does_not_synchronise(built_lib):
    from roma_amd import estimate_pose, refine_pose
    K, R, t, F, pa, pb, truth = relief_scene(n=1000, outlier_frac=0.3, noise_px=0.3)
    a, b = _dev(np.stack([pa, pa])), _dev(np.stack([pb, pb]))
    Kd = torch.as_tensor(K, device=DEV)
    seeds = torch.tensor([1, 2], device=DEV)
    counts = torch.tensor([1000, 800], device=DEV, dtype=torch.int32)
    thr = 1.0 / K[0, 0]
    R0, t0, m0, ok0 = estimate_pose(a, b, Kd, Kd, thr, seed=seeds, counts=counts, refine=True)  # warm-up: library, allocator
    refine_pose(R0, t0, a, b, Kd, Kd, thr, counts=counts, valid=ok0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        R1, t1, m1, ok1 = estimate_pose(a, b, Kd, Kd, thr, seed=seeds, counts=counts, refine=True)
        R3, t3, m3, info = refine_pose(R1, t1, a, b, Kd, Kd, thr, counts=counts, valid=ok1)
        R4, t4, m4, info4 = refine_pose(R1[0], t1[0], a[0], b[0], Kd, Kd, thr)  # the single-pair form has no ok to read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(ok1.all()) and tuple(t3.shape) == (2, 3, 1) and tuple(info4.shape) == (4,)


def test_pose_benchmark_with_refinement(built_lib):
    """the accuracy harness's device pose loop with its opt-in refined variant, on exact correspondences: the bound the
    unrefined loop is held to (test_gpu_essential.test_pose_benchmark_on_device_matches_host_path)"""
    import accuracy_harness as AH
    from test_gpu_essential import _Perfect
    aucs = []
    for seed in (0, 1):
        pair = AH.synthetic_relief_pair(120, 160, seed=seed)
        aucs.append(AH.pose_benchmark(_Perfect(pair, DEV), [pair], seed=seed, num=1500, repeats=2, pose="device", refine=True)["auc_5"])
    assert np.mean(aucs) >= 0.95, aucs
    with pytest.raises(ValueError, match="refine"):
        AH.pose_benchmark(_Perfect(pair, "cpu"), [pair], pose="host", refine=True)
