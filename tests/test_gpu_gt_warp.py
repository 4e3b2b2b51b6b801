"""roma_amd.warp_kpts / get_gt_warp / dense_metrics (csrc/gt_warp.hip) on the device against tools/gt_warp_ref.py, the numpy float64
oracle that tests/test_cpu_gt_warp.py holds to the reference's recorded outputs, on the scene of tests/gt_warp_cases.py (which has
no row within 1e-9 of a threshold, so masks and counts are compared exactly).  Both sides run the same correctly rounded
operations in the same order: the expected difference is 0, the bound 2 float64 ulps (the margin for the division sequence)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import gt_warp_cases as cases

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gt_warp_ref as gw  # noqa: E402

pytestmark = pytest.mark.gpu
ULPS = 2


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()  # a copy: the scene's arrays are read-only


def pair_args(s=None, sel=slice(None)):
    s = s or cases.scene()
    return tuple(dev(s[k][sel]) for k in ("depth0", "depth1", "T", "K0", "K1"))


def ulps(a, b):
    """worst difference of two float64 arrays in ulps, after checking that NaN and the infinities sit in the same places"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)), "NaN / inf pattern"
    f = np.isfinite(a)
    if not f.any():
        return 0.0
    return float((np.abs(a[f] - b[f]) / np.spacing(np.maximum(np.abs(a[f]), np.abs(b[f])))).max())


def same_bits(a, b):
    a, b = a.contiguous().cpu().numpy(), b.contiguous().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def device_metrics():
    """one dense_metrics call on the whole scene with maps, shared and left unchanged"""
    import roma_amd
    return roma_amd.dense_metrics(dev(cases.scene()["matches"]), *pair_args(), thresholds=cases.PCK, return_maps=True)


# ------------------------------------------------------------------------------------------------------- against the oracle
def test_warp_kpts_equals_the_oracle():
    import roma_amd
    s, o = cases.scene(), cases.oracle()
    kp = dev(s["kpts"])
    valid, warped = roma_amd.warp_kpts(kp, *pair_args(), relative_depth_error_threshold=cases.THRESHOLD)
    rel, warped2 = roma_amd.warp_kpts(kp, *pair_args(), return_relative_depth_error=True)
    assert valid.dtype == torch.bool and valid.shape == (cases.B, cases.L) and valid.is_cuda
    assert warped.dtype == torch.float64 and warped.shape == (cases.B, cases.L, 2) and rel.dtype == torch.float64
    assert same_bits(warped, warped2)
    assert np.array_equal(valid.cpu().numpy(), np.stack([w["valid"] for w in o["warp"]]))
    uw = ulps(warped.cpu().numpy(), np.stack([w["warped"] for w in o["warp"]]))
    ur = ulps(rel.cpu().numpy(), np.stack([w["rel"] for w in o["warp"]]))
    print(f"warp_kpts vs oracle: worst difference warped {uw:.2f} ulp, rel {ur:.2f} ulp")
    assert uw <= ULPS and ur <= ULPS
    # [B, 4, 4] poses and host numpy for the small matrices: the same bits
    T44 = np.concatenate([s["T"], np.broadcast_to([[[0.0, 0.0, 0.0, 1.0]]], (cases.B, 1, 4))], axis=1)
    v2, w2 = roma_amd.warp_kpts(kp, dev(s["depth0"]), dev(s["depth1"]), T44, s["K0"], s["K1"])
    assert same_bits(v2, valid) and same_bits(w2, warped)


def test_float32_and_float64_key_points_give_the_same_bits():
    import roma_amd
    kp = dev(cases.scene()["kpts"])
    for kw in (dict(), dict(return_relative_depth_error=True)):
        a, wa = roma_amd.warp_kpts(kp, *pair_args(), **kw)
        b, wb = roma_amd.warp_kpts(kp.double(), *pair_args(), **kw)
        assert same_bits(a, b) and same_bits(wa, wb)


def test_get_gt_warp_equals_warp_kpts_on_the_generated_grid():
    import roma_amd
    o = cases.oracle()
    for (H, W), key in (((None, None), "gt"), ((cases.GRID_H, cases.GRID_W), "gt_grid")):  # depth0's size, and another one
        x2, prob = roma_amd.get_gt_warp(*pair_args(), H=H, W=W)
        H, W = (cases.H0, cases.W0) if H is None else (H, W)
        assert x2.shape == (cases.B, H, W, 2) and x2.dtype == torch.float64 and prob.shape == (cases.B, H, W) and prob.dtype == torch.float32
        grid = dev(np.broadcast_to(gw.grid(H, W), (cases.B, H * W, 2)))
        valid, warped = roma_amd.warp_kpts(grid, *pair_args())
        assert same_bits(x2.reshape(cases.B, H * W, 2), warped) and same_bits(prob.reshape(cases.B, H * W), valid.float())
        assert np.array_equal(prob.cpu().numpy(), np.stack([g[1] for g in o[key]]))
        assert ulps(x2.cpu().numpy(), np.stack([g[0] for g in o[key]])) <= ULPS


def test_dense_metrics_equals_the_oracle(device_metrics):
    m, o = device_metrics, cases.oracle()["metrics"]
    assert m.n_valid.dtype == torch.int64 and m.n_below.shape == (cases.B, 3) and m.gd_sum.dtype == torch.float64
    assert m.epe.shape == () and m.pck.shape == (3,) and m.prob.dtype == torch.float32 and m.gd.dtype == torch.float64
    prob = np.stack([x["prob"] for x in o])
    assert np.array_equal(m.prob.cpu().numpy(), prob)
    assert m.n_valid.tolist() == [x["n_valid"] for x in o]
    assert np.array_equal(m.n_below.cpu().numpy(), np.stack([x["n_below"] for x in o]))
    gd = np.where(prob == 1, np.stack([x["gd"] for x in o]), np.nan)
    u = ulps(m.gd.cpu().numpy(), gd)
    # n 2^-52 sum gd: any summation order of n terms is within (n - 1) 2^-53 sum |gd| of the exact sum, taken for both sides
    worst = 0.0
    for b in range(cases.B):
        bound = o[b]["n_valid"] * 2.0 ** -52 * o[b]["gd_sum"]
        worst = max(worst, abs(float(m.gd_sum[b]) - o[b]["gd_sum"]) / bound)
        assert abs(float(m.gd_sum[b]) - o[b]["gd_sum"]) <= bound, b
    epe, pck, n, total = cases.batch_means(o)
    print(f"dense_metrics vs oracle: worst gd difference {u:.2f} ulp; gd_sum at {worst:.3f} of its bound; EPE {float(m.epe):.6f} px "
          f"(oracle {epe:.6f}), PCK {m.pck.tolist()} over {n} valid pixels")
    assert u <= ULPS
    assert abs(float(m.epe) - epe) <= n * 2.0 ** -52 * total
    assert np.array_equal(m.pck.cpu().numpy(), pck)


def test_return_maps_agree_with_the_counts(device_metrics):
    import roma_amd
    m = device_metrics
    prob, gd = m.prob.cpu().numpy(), m.gd.cpu().numpy()
    assert np.array_equal(np.isnan(gd), prob == 0) and set(np.unique(prob)) == {0.0, 1.0}
    assert m.n_valid.tolist() == [int(p.sum()) for p in prob]
    for k, thr in enumerate(cases.PCK):
        assert m.n_below[:, k].tolist() == [int((g[p == 1] < thr).sum()) for g, p in zip(gd, prob)]
    plain = roma_amd.dense_metrics(dev(cases.scene()["matches"]), *pair_args(), thresholds=cases.PCK)
    assert plain.prob is None and plain.gd is None
    for a, b in zip(plain[:5], m[:5]):
        assert same_bits(a, b)


def test_block_stride_loop_on_a_warp_larger_than_one_pass():
    """263 x 347 = 91 261 pixels: more than the 256 workgroups x 256 threads of a pair, so threads take a second pixel and the
    last pass is partial; other thresholds than the defaults"""
    import roma_amd
    s = cases.scene()
    h, w, b = 263, 347, 1
    a = (s["depth0"][b], s["depth1"][b], s["T"][b], s["K0"][b], s["K1"][b], cases.THRESHOLD)
    grid = gw.grid(h, w)
    truth = gw.warp_kpts(grid, *a)
    x2 = truth["warped"] + 0.01 * np.random.default_rng(5).standard_normal((h * w, 2))
    matches = np.concatenate([grid, x2.astype(np.float32)], axis=-1).reshape(h, w, 4)
    pck = (0.5, 1.5, 4.0)
    o = gw.dense_metrics(matches, *a, thresholds=pck)
    m = roma_amd.dense_metrics(dev(matches[None]), *pair_args(sel=slice(b, b + 1)), thresholds=pck, return_maps=True)
    assert not o["near"].any()  # a condition on the scene: no pixel at a threshold, so the masks and counts compare exactly
    assert np.array_equal(m.prob[0].cpu().numpy(), o["prob"])
    assert int(m.n_valid[0]) == o["n_valid"] and np.array_equal(m.n_below[0].cpu().numpy(), o["n_below"])
    u = ulps(m.gd[0].cpu().numpy(), np.where(o["prob"] == 1, o["gd"], np.nan))
    print(f"263 x 347 warp: worst gd difference {u:.2f} ulp over {o['n_valid']} valid pixels")
    assert u <= ULPS
    assert abs(float(m.gd_sum[0]) - o["gd_sum"]) <= o["n_valid"] * 2.0 ** -52 * o["gd_sum"]
    # the same grid generated in the warp kernel, whose loop then also takes a second pass
    x2_dev, prob_dev = roma_amd.get_gt_warp(*pair_args(sel=slice(b, b + 1)), H=h, W=w)
    assert not truth["near"].any() and np.array_equal(prob_dev[0].cpu().numpy().reshape(-1), truth["valid"].astype(np.float32))
    assert ulps(x2_dev[0].cpu().numpy().reshape(-1, 2), truth["warped"]) <= ULPS
    assert 0 < o["n_below"][0] < o["n_below"][1] < o["n_below"][2] <= o["n_valid"] and o["n_valid"] > 20000


# ------------------------------------------------------------------------------------------------ API forms and determinism
def test_strided_left_half_of_a_symmetric_warp_is_read_in_place(device_metrics):
    import roma_amd
    matches = cases.scene()["matches"]
    rng = np.random.default_rng(7)
    sym = np.concatenate([matches, rng.standard_normal(matches.shape).astype(np.float32)], axis=2)  # [B, h, 2w, 4]
    left = dev(sym)[:, :, :cases.GRID_W]
    assert not left.is_contiguous() and left.stride(-1) == 1 and left.stride(-2) == 4
    m = roma_amd.dense_metrics(left, *pair_args(), thresholds=cases.PCK, return_maps=True)
    for a, b in zip(m, device_metrics):
        assert same_bits(a, b)


def test_runs_batches_and_pair_orders_are_bit_identical(device_metrics):
    import roma_amd
    s = cases.scene()
    again = roma_amd.dense_metrics(dev(s["matches"]), *pair_args(), thresholds=cases.PCK, return_maps=True)
    for a, b in zip(again, device_metrics):  # run to run: the batch scalars too
        assert same_bits(a, b)
    kp = dev(s["kpts"])
    valid, warped = roma_amd.warp_kpts(kp, *pair_args())
    rel, _ = roma_amd.warp_kpts(kp, *pair_args(), return_relative_depth_error=True)
    for b in range(cases.B):  # B = 1 against a slice of B = 4
        sel = slice(b, b + 1)
        one = roma_amd.dense_metrics(dev(s["matches"][sel]), *pair_args(sel=sel), thresholds=cases.PCK, return_maps=True)
        for name in ("n_valid", "n_below", "gd_sum", "prob", "gd"):
            assert same_bits(getattr(one, name), getattr(device_metrics, name)[sel]), (b, name)
        v1, w1 = roma_amd.warp_kpts(kp[sel], *pair_args(sel=sel))
        r1, _ = roma_amd.warp_kpts(kp[sel], *pair_args(sel=sel), return_relative_depth_error=True)
        assert same_bits(v1, valid[sel]) and same_bits(w1, warped[sel]) and same_bits(r1, rel[sel])
    perm = [2, 0, 3, 1]
    shuffled = roma_amd.dense_metrics(dev(s["matches"][perm]), *pair_args(sel=perm), thresholds=cases.PCK, return_maps=True)
    for name in ("n_valid", "n_below", "gd_sum", "prob", "gd"):
        assert same_bits(getattr(shuffled, name), getattr(device_metrics, name)[perm]), name
    vp, wp = roma_amd.warp_kpts(kp[perm], *pair_args(sel=perm))
    assert same_bits(vp, valid[perm]) and same_bits(wp, warped[perm])


def test_a_batch_with_no_valid_pixel_gives_nan_means_and_zero_counts():
    import roma_amd
    s = cases.scene()
    d0, d1, T, K0, K1 = pair_args()
    m = roma_amd.dense_metrics(dev(s["matches"]), torch.zeros_like(d0), d1, T, K0, K1, return_maps=True)
    assert m.n_valid.tolist() == [0] * cases.B and not m.n_below.any() and m.gd_sum.tolist() == [0.0] * cases.B
    assert bool(torch.isnan(m.epe)) and bool(torch.isnan(m.pck).all())
    assert not m.prob.any() and bool(torch.isnan(m.gd).all())


def test_matcher_method_forwards():
    from roma_amd.matcher import RegressionMatcher
    import roma_amd
    a = (dev(cases.scene()["matches"]),) + pair_args()
    got = RegressionMatcher.__new__(RegressionMatcher).dense_metrics(*a, thresholds=cases.PCK)
    want = roma_amd.dense_metrics(*a, thresholds=cases.PCK)
    for x, y in zip(got[:5], want[:5]):
        assert same_bits(x, y)
