"""Device refinement of homographies and fundamental matrices (roma_amd.refine_homography / refine_fundamental,
find_*(..., lm_steps=k); csrc/model_refine.hip) against its numpy restatement tools/model_refine_ref.py; batching, determinism,
ragged and invalid pairs, NaN rows, no host synchronisation."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_model_refine import (CLEAN_THR, F, H, MAX_STEPS, NOISY_CASES, NOISY_SEEDS, clean_fits, edge_rows, error, noisy_fits,
                                   noisy_thr, scene, starts)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_refine_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# |M_device / |M_device| - M_oracle / |M_oracle||_F (sign aligned) over the 60 clean and 48 noisy fits below.  The two sides
# differ in the order of their sums and in their sin / cos / sqrt, so this is a rounding bound: ten times the worst difference
# measured on an MI355X (MEASURED), headroom for another compiler's choices.  The yardstick is the step-length stop 1e-10 on a
# unit-norm model: a last step taken by one side only leaves a few times that; orders of magnitude more would mean an accept /
# reject decision went the other way.
# H: at most 4.6e-15 over its 54 fits (both sides take the same steps).  F: 1e-18 - 1e-14 on 50 fits and 2.5e-11 - 2.2e-10 on
# four noisy ones, where one side takes a last step the other does not.
MEASURED = 2.2e-10  # noisy F 1.0 px / 30 % / seed 5: the oracle takes a seventh step of that length, the device stops after six
TOL = 10 * MEASURED


def _dev(x, dtype=np.float32):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _fn(model):
    import roma_amd
    return roma_amd.refine_homography if model == H else roma_amd.refine_fundamental


def _refine(model, M, pa, pb, thr, **kw):
    return _fn(model)(_dev(M, np.float64), _dev(pa), _dev(pb), thr, **kw)


def _unit_diff(A, B):
    """|A / |A| - B / |B||_F with the sign aligned"""
    A, B = np.asarray(A) / np.linalg.norm(A), np.asarray(B) / np.linalg.norm(B)
    return float(min(np.linalg.norm(A - B), np.linalg.norm(A + B)))


def _error_bound(model, Mo, frac, noise):
    """what TOL on the unit-norm model is in pixels of the case's error, to first order: TOL x the norm of the gradient of the
    error by the nine entries of the unit-norm model (central differences), doubled for the second order"""
    U = np.asarray(Mo) / np.linalg.norm(Mo)
    g = np.zeros(9)
    for k in range(9):
        d = np.zeros(9)
        d[k] = 1e-7
        g[k] = (error(model, U + d.reshape(3, 3), frac, noise) - error(model, U - d.reshape(3, 3), frac, noise)) / 2e-7
    return 2 * TOL * float(np.linalg.norm(g))


@pytest.mark.parametrize("model", [H, F])
def test_device_matches_the_oracle(built_lib, model):
    """items 8 and 13: every clean and noisy fit against the oracle - model, steps, active rows, mask, cost, and the case's
    error in pixels"""
    worst, worst_name = 0.0, ""
    fails = []
    for name, Ms, pa, pb, thr, frac, noise in clean_fits(model) + noisy_fits(model):
        o = mr.refine(model, Ms, pa, pb, thr, MAX_STEPS)
        M, mask, info, cost = _refine(model, Ms, pa, pb, thr, max_steps=MAX_STEPS)
        assert M.dtype == torch.float64 and tuple(M.shape) == (3, 3) and mask.dtype == torch.bool and info.dtype == torch.int32
        assert tuple(cost.shape) == (2,) and cost.dtype == torch.float64
        M, mask, got, cost = M.cpu().numpy(), mask.cpu().numpy(), info.cpu().tolist(), cost.cpu().numpy()
        d = _unit_diff(M, o["M"])
        e_dev, e_orc = error(model, M, frac, noise), error(model, o["M"], frac, noise)
        bound = _error_bound(model, o["M"], frac, noise)
        if d > worst:
            worst, worst_name = d, name
        print(f"{name}: diff {d:.3e} info {got} oracle {o['info']} cost {cost[1]:.9e} oracle {o['cost']:.9e} "
              f"error {e_dev:.6e} oracle {e_orc:.6e} bound {bound:.2e}")
        # rows whose error sits at the threshold may fall either way; the oracle shows that these cases have none
        assert edge_rows(model, o["M"], pa, pb, thr) == 0
        if not np.array_equal(mask, o["mask"]):
            fails.append((name, "mask"))
        # a last step at the step-length stop may be taken by one side only; the active rows and the flag are the same
        if not (abs(got[0] - o["info"][0]) <= 1 and got[2:] == list(o["info"][2:])):
            fails.append((name, "info", got, o["info"]))
        # the start's cost differs by the order of the sums only; the final one also by the last step, so it is printed
        if not (cost[1] <= cost[0] and abs(cost[0] - o["cost0"]) <= 1e-9 * o["cost0"]):
            fails.append((name, "cost", cost.tolist(), o["cost0"], o["cost"]))
        if not abs(e_dev - e_orc) <= bound + 1e-12:
            fails.append((name, "error", e_dev, e_orc, bound))
    print(f"worst difference {worst:.3e} ({worst_name})")
    assert not fails, fails
    assert worst <= TOL, (worst, worst_name)


@pytest.mark.parametrize("model", [H, F])
def test_degenerate_starts_return_the_input(built_lib, model):
    M0, pa, pb, truth, _ = scene(model, 0.0)
    pa, pb = mr.as_f32(pa), mr.as_f32(pb)
    shift = np.eye(3)
    shift[0, 2] = 50.0
    Ms = shift @ M0 if model == H else np.linalg.inv(shift).T @ M0
    thr = CLEAN_THR[model]
    o = mr.refine(model, Ms, pa, pb, thr)
    assert o["info"][0] == 0 and o["info"][2] < mr.MIN_ROWS[model]
    M, mask, info, cost = _refine(model, Ms, pa, pb, thr)
    assert np.array_equal(M.cpu().numpy(), Ms) and info.cpu().tolist() == list(o["info"])
    assert np.array_equal(mask.cpu().numpy(), o["mask"]) and float(cost[0]) == float(cost[1])
    M, mask, info, cost = _refine(model, 2 * M0, pa, pb, thr, max_steps=0)
    assert np.array_equal(M.cpu().numpy(), 2 * M0) and info.cpu().tolist() == [0, 1, int(truth.sum()), 1]
    for bad in (np.zeros((3, 3)), M0 * np.nan):
        M, mask, info, cost = _refine(model, bad, pa, pb, thr)
        assert np.array_equal(M.cpu().numpy(), bad, equal_nan=True) and info.cpu().tolist() == [0, 0, 0, 0]
        assert not bool(mask.any()) and bool(torch.isnan(cost).all())


def _noisy(model, noise=0.3, frac=0.3):
    _, pa, pb, _, _ = scene(model, frac, noise)
    name, Ms, pa, pb, thr, _, _ = [f for f in noisy_fits(model) if f[5] == frac and f[6] == noise][0]
    return Ms, pa, pb, thr


@pytest.mark.parametrize("model", [H, F])
def test_results_are_bit_identical_alone_in_a_batch_and_over_repeats(built_lib, model):
    """item 9: the same pair alone, at two places of a batch of 8 among other pairs, and over 20 calls"""
    Ms, pa, pb, thr = _noisy(model)
    others = [f for f in noisy_fits(model) if f[4] == thr][:8]
    single = _refine(model, Ms, pa, pb, thr)
    assert int(single[2][0]) >= 1
    Mb = np.stack([f[1] for f in others])
    Pa, Pb = np.stack([f[2] for f in others]), np.stack([f[3] for f in others])
    for place in (2, 7):
        Mb[place], Pa[place], Pb[place] = Ms, pa, pb
    batch = _refine(model, Mb, Pa, Pb, thr)
    for place in (2, 7):
        assert all(torch.equal(s, b[place]) for s, b in zip(single, batch))
    for _ in range(20):
        again = _refine(model, Mb, Pa, Pb, thr)
        assert all(torch.equal(x, y) for x, y in zip(batch, again))


@pytest.mark.parametrize("model", [H, F])
def test_ragged_counts_invalid_pairs_nan_rows_and_small_inputs(built_lib, model):
    """item 10"""
    Ms, pa, pb, thr = _noisy(model)
    n, k = len(pa), mr.MIN_ROWS[model]
    counts = [n, n - 100, n - 300, 1500, 1000, 700, k - 1, n]
    a = np.full((8, n, 2), np.nan)
    b = np.full((8, n, 2), np.nan)
    for i, c in enumerate(counts):
        a[i, :c], b[i, :c] = pa[:c], pb[:c]
    Mb = np.stack([Ms * (1 + i) for i in range(8)])  # the scale of the input is free
    valid = torch.tensor([True] * 7 + [False])
    cd = torch.tensor(counts)
    M, mask, info, cost = _refine(model, Mb, a, b, thr, counts=cd, valid=valid)
    assert bool((info[:6, 0] > 0).all()) and info[:, 3].cpu().tolist() == [1] * 6 + [0, 0]
    for i in range(8):
        c = counts[i]
        assert not bool(mask[i, c:].any())
        if i >= 6:  # fewer rows than the model needs / not valid: copied through bit for bit
            assert np.array_equal(M[i].cpu().numpy(), Mb[i]) and not bool(mask[i].any())
            assert info[i].cpu().tolist() == [0, 0, 0, 0] and bool(torch.isnan(cost[i]).all())
            continue
        Mi, mi, ii, ci = _refine(model, Mb[i], a[i, :c], b[i, :c], thr)
        assert torch.equal(Mi, M[i]) and torch.equal(mi, mask[i, :c]) and torch.equal(ii, info[i]) and torch.equal(ci, cost[i])
        o = mr.refine(model, Mb[i], pa[:c], pb[:c], thr)
        assert _unit_diff(Mi.cpu().numpy(), o["M"]) <= TOL and abs(int(ii[0]) - o["info"][0]) <= 1 and int(ii[2]) == o["info"][2]
    # NaN rows are never active: the same pair with those rows removed, up to the order of the sums
    rows = np.array([0, 17, 400, n - 1])
    a2, b2 = pa.copy(), pb.copy()
    a2[rows[:2]] = np.nan
    b2[rows[2:], 1] = np.nan
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    M1, m1, i1, c1 = _refine(model, Ms, a2, b2, thr)
    M2, m2, i2, c2 = _refine(model, Ms, pa[keep], pb[keep], thr)
    assert _unit_diff(M1.cpu().numpy(), M2.cpu().numpy()) <= TOL and not bool(m1[rows].any())
    assert torch.equal(m1[keep], m2) and int(i1[2]) == int(i2[2]) and abs(int(i1[0]) - int(i2[0])) <= 1
    # thr = inf: plain least squares over the finite rows, every one of them active
    o = mr.refine(model, Ms, a2, b2, math.inf)
    M3, m3, i3, c3 = _refine(model, Ms, a2, b2, math.inf)
    assert _unit_diff(M3.cpu().numpy(), o["M"]) <= TOL and int(i3[2]) == n - 4 == o["info"][2] and int(i3[0]) >= 1
    assert np.array_equal(m3.cpu().numpy(), keep) and math.isfinite(float(c3[1])) and float(c3[1]) < float(c3[0])
    # fewer rows than the model needs, and no pairs at all: nothing is launched
    M4, m4, i4, c4 = _refine(model, Ms, pa[:k - 1], pb[:k - 1], thr)
    assert np.array_equal(M4.cpu().numpy(), Ms) and i4.cpu().tolist() == [0, 0, 0, 0] and not bool(m4.any())
    M5, m5, i5, c5 = _refine(model, np.zeros((0, 3, 3)), np.zeros((0, 10, 2)), np.zeros((0, 10, 2)), thr)
    assert tuple(M5.shape) == (0, 3, 3) and tuple(m5.shape) == (0, 10) and tuple(i5.shape) == (0, 4) and tuple(c5.shape) == (0, 2)


@pytest.mark.parametrize("model", [H, F])
def test_counts_around_a_wave_the_workgroup_and_the_minimum(built_lib, model):
    """one batch whose counts leave threads and whole waves of the workgroup without rows, put one row past a wave (64) and
    past the workgroup (512), and end at MIN_ROWS and one below it; exact data, a start 1e-4 off"""
    M0, pa, pb, _, _ = scene(model, 0.0)
    pa, pb = mr.as_f32(pa), mr.as_f32(pb)
    Ms, thr, k = starts(model, M0)[0], CLEAN_THR[model], mr.MIN_ROWS[model]
    n, counts = 1000, [513, 512, 511, 65, 64, 63, k, k - 1]
    a = np.full((8, n, 2), np.nan)
    b = np.full((8, n, 2), np.nan)
    for i, c in enumerate(counts):
        a[i, :c], b[i, :c] = pa[:c], pb[:c]
    cd = torch.tensor(counts)
    out = _refine(model, np.stack([Ms] * 8), a, b, thr, counts=cd)
    again = _refine(model, np.stack([Ms] * 8), a, b, thr, counts=cd)
    # the costs of the pair that is not fitted are NaN
    assert all(torch.equal(x, y) for x, y in zip(out[:3], again[:3])) and torch.equal(out[3][:7], again[3][:7])
    M, mask, info, cost = out
    for i, c in enumerate(counts):
        Mi, mi, ii, ci = _refine(model, Ms, pa[:c], pb[:c], thr)
        assert torch.equal(Mi, M[i]) and torch.equal(mi, mask[i, :c]) and torch.equal(ii, info[i]), c
        assert not bool(mask[i, c:].any())
        Md, got = M[i].cpu().numpy(), info[i].cpu().tolist()
        print(f"count {c}: info {got} cost {cost[i].cpu().tolist()}")
        if c >= 63:
            assert torch.equal(ci, cost[i])
            o = mr.refine(model, Ms, pa[:c], pb[:c], thr)
            assert o["info"][0] >= 1 and edge_rows(model, o["M"], pa[:c], pb[:c], thr) == 0
            d = _unit_diff(Md, o["M"])
            print(f"count {c}: diff {d:.3e} oracle {o['info']}")
            assert d <= TOL, (c, d)
            assert np.array_equal(mask[i, :c].cpu().numpy(), o["mask"]) and got[2:] == list(o["info"][2:]), (c, got, o["info"])
        elif c == k:
            assert torch.equal(ci, cost[i]) and got[3] == 1 and float(cost[i, 1]) <= float(cost[i, 0])
            assert mr.pixel_cost(model, Md, pa[:c], pb[:c], thr)[0] <= mr.pixel_cost(model, Ms, pa[:c], pb[:c], thr)[0]
        else:  # fewer rows than the model needs: untouched
            assert np.array_equal(Md, Ms) and got == [0, 0, 0, 0] and not bool(mask[i].any()) and bool(torch.isnan(cost[i]).all())


@pytest.mark.parametrize("model", [H, F])
@pytest.mark.parametrize("method", ["ransac", "magsac"])
def test_find_with_lm_steps_is_find_then_refine_and_the_default_is_unchanged(built_lib, model, method):
    """item 11"""
    import roma_amd
    from roma_amd import geometry as G
    find = roma_amd.find_homography if model == H else roma_amd.find_fundamental
    _, pa, pb, _, _ = scene(model, 0.3, 0.3)
    n = len(pa)
    a, b = np.stack([pa] * 4), np.stack([pb] * 4)
    a[3], b[3] = np.nan, np.nan  # a pair without a model
    a, b = _dev(a), _dev(b)
    seeds = torch.arange(4) + 1
    counts = torch.tensor([n, n - 200, 900, n])
    thr = 1.0
    M0, m0, ok0 = find(a, b, thr, seed=seeds, counts=counts, method=method)
    M1, m1, ok1 = find(a, b, thr, seed=seeds, counts=counts, method=method, lm_steps=10)
    assert ok0.cpu().tolist() == [True, True, True, False] and torch.equal(ok0, ok1)
    M2, m2, info, cost = _fn(model)(M0, a, b, thr, max_steps=10, counts=counts)
    assert torch.equal(M1, M2) and torch.equal(m1, m2) and bool((info[:3, 0] > 0).all()) and info[:, 3].cpu().tolist() == [1, 1, 1, 0]
    assert torch.equal(M1[3], M0[3]) and not bool(m1[3].any()) and bool((cost[:3, 1] < cost[:3, 0]).all())
    # the single-pair form
    Ms, ms = find(a[0], b[0], thr, seed=1, method=method, lm_steps=10)
    assert torch.equal(Ms, M1[0]) and torch.equal(ms, m1[0])
    assert find(a[3], b[3], thr, seed=1, method=method, lm_steps=10) == (None, None)
    # without the keyword, and with lm_steps=0: the outputs of ransac() / magsac() as before
    conf, iters = ((0.995, 2000), (0.99, 1000))[model]
    if method == "ransac":
        raw = G.ransac(model, a, b, thr, conf, iters, seeds, True, counts)[:3]
    else:
        raw = G.magsac(model, a, b, thr, conf, iters, seeds, 10, counts)[:3]
    for got in ((M0, m0, ok0), find(a, b, thr, seed=seeds, counts=counts, method=method, lm_steps=0)):
        assert all(torch.equal(x, y) for x, y in zip(got, raw))


def test_batched_refinement_does_not_synchronise(built_lib):
    """item 12"""
    import roma_amd
    for model in (H, F):
        find = roma_amd.find_homography if model == H else roma_amd.find_fundamental
        _, pa, pb, _, _ = scene(model, 0.3, 0.3)
        a, b = _dev(np.stack([pa, pa])), _dev(np.stack([pb, pb]))
        seeds = torch.tensor([1, 2], device=DEV)
        counts = torch.tensor([len(pa), 800], device=DEV, dtype=torch.int32)
        M0, m0, ok0 = find(a, b, 1.0, seed=seeds, counts=counts, lm_steps=10)  # warm-up: library, allocator
        _fn(model)(M0, a, b, 1.0, counts=counts, valid=ok0)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            M1, m1, ok1 = find(a, b, 1.0, seed=seeds, counts=counts, lm_steps=10)
            M2, m2, ok2 = find(a, b, 1.0, seed=seeds, counts=counts, method="magsac", lm_steps=10)
            M3, m3, info, cost = _fn(model)(M1, a, b, 1.0, counts=counts, valid=ok1)
            M4, m4, info4, cost4 = _fn(model)(M1[0], a[0], b[0], 1.0)  # the single-pair form has no ok to read
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert bool(ok1.all()) and tuple(M3.shape) == (2, 3, 3) and tuple(info4.shape) == (4,) and tuple(cost4.shape) == (2,)
