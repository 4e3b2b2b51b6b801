"""roma_amd.pose_error / homography_corner_error / pose_auc / ErrorLog (csrc/metrics.hip) on the device against tools/metrics_ref.py,
the numpy float64 restatement that tests/test_cpu_metrics.py holds to the reference's recorded outputs, on the cases of
tests/metrics_cases.py.  Both sides run the same correctly rounded operations in the same order, so the cosines are bit-equal and
only the two acos implementations differ: the angles are bounded in ulps (ANGLE_ULPS, the measurement in DESIGN.md section 10
rounded up to a power of two); the corner error has no transcendental - expected 0, bound 2 ulps; counts are exact."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_geometry import _homography_scene, relief_scene

import metrics_cases as cases

sys.path.insert(0, os.path.join(ROOT, "tools"))
import metrics_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
ANGLE_ULPS = 2  # measured on the MI355X: 2.00 ulps of the angle as acos returns it; at most 8
CORNER_ULPS = 2  # measured: 0
GUARD = 8


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()  # a copy: the cases' arrays are read-only


def ulps(a, b, unit=None):
    """worst difference of two float64 arrays in ulps (of the larger of the two, or in the units given), after checking that NaN
    and the infinities sit in the same places"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)), "NaN / inf pattern"
    f = np.isfinite(a)
    if not f.any():
        return 0.0
    unit = np.spacing(np.maximum(np.abs(a), np.abs(b))) if unit is None else np.broadcast_to(unit, a.shape)
    return float((np.abs(a[f] - b[f]) / unit[f]).max())


def same_bits(a, b):
    a, b = a.contiguous().cpu().numpy(), b.contiguous().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def pose_args(B):
    p = cases.pose_cases()
    return dev(p["R"][:B]), dev(p["t"][:B]), dev(p["T"][:B]), dev(p["ok"][:B]).bool()


def corner_args(B):
    c = cases.corner_cases()
    return dev(c["Hp"][:B]), dev(c["Hg"][:B]), dev(c["sizes"][:B]), dev(c["ok"][:B]).bool()


# ------------------------------------------------------------------------------------------------------ errors against the oracle
@pytest.mark.parametrize("B", cases.BATCHES)
def test_pose_error_equals_the_restatement(B):
    import roma_amd
    p, want = cases.pose_cases(), cases.oracle()["pose"][:B]
    R, t, T, ok = pose_args(B)
    e = roma_amd.pose_error(R, t, T, ok=ok)
    assert all(x.shape == (B,) and x.dtype == torch.float64 and x.is_cuda for x in e)
    got = torch.stack(tuple(e), dim=1).cpu().numpy()
    u = ulps(got, want, cases.oracle()["pose_unit"][:B])
    print(f"pose_error B = {B}: worst difference {u:.2f} ulp of the angle")
    assert u <= ANGLE_ULPS
    # special values are exact: 0, 90, 180, the 90s of a pair without a pose, NaN where the oracle has it (checked by ulps)
    for b, kind in enumerate(p["kind"][:B]):
        if kind != "spread":
            exact = {"same_exact": (0, 1, 2), "pi": (1, 2), "antiparallel": (0,), "orthogonal": (0,), "not_ok": (0, 1, 2)}.get(kind, ())
            for i in exact:
                assert got[b, i] == want[b, i], (b, kind, i)
    assert np.array_equal(got[:, 2][~np.isnan(got[:, 0])], np.maximum(got[:, 0], got[:, 1])[~np.isnan(got[:, 0])])
    # t as estimate_pose returns it, [B, 3, 1], the [B, 4, 4] form of T and host numpy for it: the same bits
    T44 = np.concatenate([p["T"][:B], np.broadcast_to([[[0.0, 0.0, 0.0, 1.0]]], (B, 1, 4))], axis=1)
    e2 = roma_amd.pose_error(R, t[:, :, None], T44, ok=ok)
    assert all(same_bits(x, y) for x, y in zip(e, e2))


def test_pose_error_without_ok_and_the_unbatched_and_reference_forms():
    import roma_amd
    p, want = cases.pose_cases(), cases.oracle()["pose"]
    R, t, T, ok = pose_args(65)
    rows = [b for b in range(65) if p["ok"][b]]
    plain = torch.stack(tuple(roma_amd.pose_error(R[rows], t[rows], T[rows])), dim=1).cpu().numpy()  # ok=None: every pair has a pose
    assert ulps(plain, want[rows], cases.oracle()["pose_unit"][rows]) <= ANGLE_ULPS
    one = roma_amd.pose_error(R[0], t[0], T[0])
    assert all(x.shape == () for x in one) and same_bits(torch.stack(tuple(one)), torch.stack(tuple(roma_amd.pose_error(R[:1], t[:1], T[:1])), dim=1)[0])
    e_t, e_R = roma_amd.compute_pose_error(T[0], R[0], t[0])
    assert same_bits(e_t, one.e_t) and same_bits(e_R, one.e_R)
    # a pair without a pose: 90 whatever R and t hold
    garbage = torch.full((3, 3, 3), float("nan"), device="cuda", dtype=torch.float64)
    e = roma_amd.pose_error(garbage, garbage[:, 0], T[:3], ok=torch.zeros(3, dtype=torch.bool, device="cuda"))
    assert torch.stack(tuple(e)).tolist() == [[90.0] * 3] * 3


@pytest.mark.parametrize("B", cases.BATCHES)
def test_corner_error_equals_the_restatement(B):
    import roma_amd
    c, want = cases.corner_cases(), cases.oracle()["corner"][:B]
    Hp, Hg, sizes, ok = corner_args(B)
    e = roma_amd.homography_corner_error(Hp, Hg, sizes, ok=ok)
    assert e.shape == (B,) and e.dtype == torch.float64 and e.is_cuda
    u = ulps(e.cpu().numpy(), want)
    print(f"homography_corner_error B = {B}: worst difference {u:.2f} ulp")
    assert u <= CORNER_ULPS
    e2 = roma_amd.homography_corner_error(Hp, c["Hg"][:B], c["sizes"][:B], ok=ok)  # host numpy for the ground truth
    assert same_bits(e, e2)
    if B >= 7:
        # ok == 0: the fallback matrix whatever H_pred holds, NaN included
        other = Hp.clone()
        other[~ok] = 12345.0
        assert same_bits(e, roma_amd.homography_corner_error(other, Hg, sizes, ok=ok))
        one = roma_amd.homography_corner_error(Hp[5], Hg[5], sizes[5])
        assert one.shape == () and same_bits(one, roma_amd.homography_corner_error(Hp[5:6], Hg[5:6], sizes[5:6])[0])


# ------------------------------------------------------------------------------------------------------------------ the log
def test_appends_of_1_5_257_rows_leave_the_bits_of_one_append_of_263():
    import roma_amd
    R, t, T, ok = pose_args(257)
    want = cases.oracle()["pose"][:, 2]
    pieces = roma_amd.ErrorLog(capacity=300)
    extra = dev(np.array([1.5, 2.5, 3.5, 4.5, 5.5, 90.0]))
    pieces.append(extra[:1])
    pieces.append(extra[1:])
    roma_amd.pose_error(R, t, T, ok=ok, log=pieces)
    whole = roma_amd.ErrorLog(capacity=300)
    e_pose = roma_amd.pose_error(R, t, T, ok=ok).e_pose
    whole.append(torch.cat((extra, e_pose)))
    assert pieces.errors().shape == (263,) and same_bits(pieces.errors(), whole.errors())
    assert same_bits(pieces._rows, whole._rows) and pieces._state.tolist() == whole._state.tolist() == [263, 0]
    assert ulps(pieces.errors()[6:].cpu().numpy(), want, cases.oracle()["pose_unit"][:, 2]) <= ANGLE_ULPS
    a, b = pieces.summary(cases.POSE_THRESHOLDS), whole.summary(cases.POSE_THRESHOLDS)
    assert all(same_bits(x, y) for x, y in zip(a, b)) and int(a.n) == 263 and int(a.dropped) == 0
    assert pieces.pose_summary() == whole.pose_summary() == mr.pose_summary(pieces.errors().cpu().numpy())
    # the corner error appends the same way
    Hp, Hg, sizes, okc = corner_args(65)
    log = roma_amd.ErrorLog(capacity=100)
    e = roma_amd.homography_corner_error(Hp[:1], Hg[:1], sizes[:1], ok=okc[:1], log=log)
    e2 = roma_amd.homography_corner_error(Hp[1:], Hg[1:], sizes[1:], ok=okc[1:], log=log)
    assert same_bits(log.errors(), torch.cat((e, e2))) and log._state.tolist() == [65, 0]


def test_a_full_log_keeps_the_first_rows_counts_the_rest_and_leaves_the_guard_alone():
    import roma_amd
    R, t, T, ok = pose_args(257)
    log = roma_amd.ErrorLog(capacity=260)
    buffer = torch.full((260 + GUARD,), -7.0, device="cuda", dtype=torch.float64)
    log._rows = buffer[:260]  # the log's rows with guard rows behind them
    extra = dev(np.array([1.5, 2.5, 3.5, 4.5, 5.5, 90.0]))
    log.append(extra[:1]).append(extra[1:])
    e_pose = roma_amd.pose_error(R, t, T, ok=ok, log=log).e_pose
    assert log._state.tolist() == [263, 3]
    assert same_bits(buffer[:260], torch.cat((extra, e_pose))[:260]) and buffer[260:].tolist() == [-7.0] * GUARD
    log.append(extra)  # a log that is already full: everything is dropped, nothing is written
    assert log._state.tolist() == [269, 9] and buffer[260:].tolist() == [-7.0] * GUARD
    s = log.summary(cases.POSE_THRESHOLDS)
    assert int(s.n) == 260 and int(s.dropped) == 9
    with pytest.raises(roma_amd._lib.RomaHipError, match="dropped 9"):
        log.pose_summary()
    with pytest.raises(roma_amd._lib.RomaHipError, match="dropped 9"):
        log.homography_summary()


# -------------------------------------------------------------------------------------------------------------- the summary
@pytest.mark.parametrize("name", ["n0", "n1", "n2", "n255", "n256", "n257", "n7500", "n65536", "none_below"])
def test_summary_equals_the_restatement(name):
    import roma_amd
    e = cases.error_sets()[name]
    n = e.size
    assert f"n{n}" == name or name == "none_below"
    log = roma_amd.ErrorLog(capacity=max(n, 1))
    d = dev(e)
    for at in range(0, n, 65535):
        log.append(d[at:at + 65535])
    for thr in (cases.POSE_THRESHOLDS, cases.HOMOGRAPHY_THRESHOLDS):
        want = cases.oracle()["summary"][name][thr]
        s = log.summary(thr)
        again = log.summary(thr)
        assert all(same_bits(x, y) for x, y in zip(s, again))  # run to run
        auc = roma_amd.pose_auc(d, thr)
        assert same_bits(auc, s.auc)  # the host count and the device cursor: the same launch shape, the same bits
        assert int(s.n) == n and int(s.dropped) == 0 and s.below.tolist() == want["below"]
        acc, got = s.acc.cpu().numpy(), s.auc.cpu().numpy()
        if n == 0:
            assert np.isnan(acc).all() and np.isnan(got).all()
            continue
        assert np.array_equal(acc, np.array(want["below"], dtype=np.float64) / np.float64(n))
        ref = np.array(want["auc"])
        worst = float(np.max(np.abs(got - ref) / np.where(ref == 0, 1.0, np.abs(ref))))
        print(f"summary {name} T = {len(thr)}: worst relative auc difference {worst:.3e} (bound {cases.auc_bound(n):.3e})")
        assert np.all(np.abs(got - ref) <= cases.auc_bound(n) * np.abs(ref))
    if n:
        assert log.pose_summary() == mr.pose_summary(e)  # the restatement reduces in the device's order: the same bits
        assert log.homography_summary().keys() == mr.homography_summary(e).keys()


def test_more_than_65536_errors_are_refused():
    import roma_amd
    from roma_amd import _lib
    e = torch.zeros(65537, device="cuda", dtype=torch.float64)
    with pytest.raises(ValueError, match="65536"):
        roma_amd.pose_auc(e, (5.0,))
    lib = _lib.load()
    out = torch.zeros(4, device="cuda", dtype=torch.float64)
    import ctypes as C
    rc = lib.roma_op_error_summary(e.data_ptr(), 65537, None, 0, (C.c_double * 1)(5.0), 1, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                   out.data_ptr(), None)
    assert rc != 0 and "65536" in _lib.last_error(lib)
    assert same_bits(roma_amd.pose_auc(e[:65536], (5.0,)), torch.tensor([1.0], dtype=torch.float64))  # all zeros: the whole area


# ------------------------------------------------------------------------------------------------------------------ chains
def test_pose_chain_equals_the_host_route():
    """estimate_pose (five seeds) -> pose_error(log=) -> pose_summary() against reading R, t, ok back and scoring them with the
    restatement"""
    import roma_amd
    K, Rg, tg, F, pa, pb, _ = relief_scene()
    B = 5
    a, b = dev(np.broadcast_to(pa, (B,) + pa.shape)), dev(np.broadcast_to(pb, (B,) + pb.shape))
    T = np.broadcast_to(np.concatenate([Rg, tg[:, None]], axis=1), (B, 3, 4))
    log = roma_amd.ErrorLog()
    R, t, mask, ok = roma_amd.estimate_pose(a, b, K, K, 0.5 / K[0, 0], seed=torch.arange(1, B + 1))
    e = roma_amd.pose_error(R, t, T, ok=ok, log=log)
    log.append(e.e_pose[-1:])  # the ScanNet loop's second copy of the last repeat
    got = log.pose_summary()
    host = mr.pose_errors(R.cpu().numpy(), t.cpu().numpy(), T, ok.cpu().numpy())
    assert ok.all() and np.isfinite(host).all() and host[:, 2].min() > 0.0  # poses were found: the scores are not the fallback's
    unit = np.array([[np.spacing(x) for x in mr.pose_angles(R[i].cpu().numpy(), t[i].cpu().numpy(), T[i])] for i in range(B)])
    assert ulps(torch.stack(tuple(e), dim=1).cpu().numpy(), host, np.concatenate([unit, unit.max(axis=1, keepdims=True)], axis=1)) <= ANGLE_ULPS
    device_errors = log.errors().cpu().numpy()
    assert device_errors.shape == (B + 1,) and device_errors[-1] == device_errors[-2]
    want = mr.pose_summary(np.append(host[:, 2], host[-1, 2]))
    assert got.keys() == want.keys() and got == mr.pose_summary(device_errors)
    for k in want:
        # the two routes' errors differ by ANGLE_ULPS ulps at the most, 1e-15 relative; (L t - S) cancels to no less than a thousandth
        # of its terms unless every error lies within 0.1 % of a threshold
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    assert 0.0 < got["auc_20"] <= 1.0


def test_homography_chain_equals_the_host_route():
    import roma_amd
    Hg, pa, pb, _ = _homography_scene()
    B = 5
    a, b = dev(np.broadcast_to(pa, (B,) + pa.shape)), dev(np.broadcast_to(pb, (B,) + pb.shape))
    sizes = np.broadcast_to([864.0, 864.0, 864.0, 700.0], (B, 4))
    Hgt = np.broadcast_to(Hg, (B, 3, 3))
    log = roma_amd.ErrorLog()
    H, mask, ok = roma_amd.find_homography(a, b, 3.0, seed=torch.arange(1, B + 1))
    e = roma_amd.homography_corner_error(H, Hgt, sizes, ok=ok, log=log)
    got = log.homography_summary()
    host = mr.corner_errors(H.cpu().numpy(), Hgt, sizes, ok.cpu().numpy())
    assert ok.all() and np.isfinite(host).all() and host.max() > 0.0
    assert ulps(e.cpu().numpy(), host) <= CORNER_ULPS
    want = mr.homography_summary(host)
    assert got == mr.homography_summary(log.errors().cpu().numpy())
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    assert 0.0 < got["hpatches_homog_auc_10"] <= 1.0
