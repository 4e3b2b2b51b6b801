"""tools/metrics_ref.py (the oracle of roma_amd.pose_error / homography_corner_error / pose_auc / ErrorLog) against what the unmodified
reference returned on the cases of tests/metrics_cases.py (tests/golden/metrics_reference.npz), the exact special values, the closed
form of pose_auc against its sort-and-trapezoid form, and the C ABI and Python surface of the four roma_op_* entries (dlopen
only).  No GPU."""
import glob
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import metrics_cases as cases

sys.path.insert(0, os.path.join(ROOT, "tools"))
import metrics_ref as mr  # noqa: E402

NEW_SYMBOLS = ("roma_op_pose_error", "roma_op_corner_error", "roma_op_error_log_append", "roma_op_error_summary")
# restatement against reference on the rows whose angles lie in [1, 179] degrees: both form the cosine from the same nine (three)
# products, the reference through BLAS in another order - a few ulps of a cosine, 4 x 2.2e-16, times 1 / sin(1 deg) = 57.3 rad per
# unit of cosine, times 57.3 degrees per rad: 3e-12 degrees
POSE_ATOL_DEG = 1e-11


def rel_close(a, b, bound):
    """|a - b| <= bound |b| element by element, NaN only where both are"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(a)] <= bound * np.abs(b)[~np.isnan(a)]))


# ------------------------------------------------------------------------------------------------- oracle against the golden
def test_recorded_pose_rows_are_the_generated_ones():
    """the golden holds the bits the reference ran on; the generator reproduces them up to this machine's libm"""
    g, p = cases.golden(), cases.pose_cases()
    n = cases.GOLDEN_POSE_ROWS
    for k in ("R", "t", "T"):
        assert g["in_" + k].shape == p[k][:n].shape and np.allclose(g["in_" + k], p[k][:n], rtol=1e-12, atol=1e-12, equal_nan=True), k
    assert np.array_equal(g["in_ok"], p["ok"][:n])
    assert p["kind"][0] == "spread" and p["kind"][1:1 + len(cases.SPECIAL_KINDS)] == cases.SPECIAL_KINDS
    assert len(p["kind"]) == cases.N_POSE == max(cases.BATCHES)


def test_error_sets_are_generated_bit_for_bit_and_hold_what_they_should():
    g, sets = cases.golden(), cases.error_sets()
    assert [sets[f"n{n}"].size for n in cases.SET_SIZES] == list(cases.SET_SIZES)
    for name, e in sets.items():
        assert int(g["chk_" + name]) == cases.checksum(e), name  # integer arithmetic only: the same bits on every machine
        assert not (e < 0).any()
    for n in cases.SET_SIZES[3:]:
        e = sets[f"n{n}"]
        for v in (0.0, 5.0, 10.0, 15.0, 20.0, 90.0, np.inf):
            assert (e == v).sum() >= 1, (n, v)
        assert np.isnan(e).sum() == 2 and (e == 0.0).sum() >= 2
        finite = e[np.isfinite(e)]
        assert np.unique(finite).size < finite.size  # ties
        assert 0.05 < (e < 5.0).mean() < 0.5
    assert not (sets["none_below"] < 25.0).any() and np.isnan(sets["none_below"]).any() and np.isinf(sets["none_below"]).any()


def test_pose_error_restatement_matches_the_reference():
    g, p = cases.golden(), cases.pose_cases()
    n = cases.GOLDEN_POSE_ROWS
    mine = mr.pose_errors(g["in_R"], g["in_t"], g["in_T"], g["in_ok"])
    worst = 0.0
    seen = 0
    for b in range(n):
        kind = p["kind"][b]
        if kind == "not_ok":
            assert np.isnan(g["ref_e_t"][b]) and tuple(mine[b]) == (90.0, 90.0, 90.0)  # never reaches the reference
            continue
        ref_t, ref_R = float(g["ref_e_t"][b]), float(g["ref_e_R"][b])
        assert math.isnan(ref_t) == math.isnan(mine[b, 0]) == (kind == "zero_t"), (b, kind)
        assert mine[b, 2] == max(mine[b, 0], mine[b, 1]) or math.isnan(mine[b, 2])
        if kind == "spread":  # every angle in [1, 179] degrees (e_t folded to [1, 90])
            assert 0.99 < ref_t <= 90.0 and 0.99 < ref_R < 179.01, (b, ref_t, ref_R)
            worst = max(worst, abs(mine[b, 0] - ref_t), abs(mine[b, 1] - ref_R))
            seen += 1
        else:  # the component a special row is about has an exact cosine: the same bits on both sides
            exact = {"same_exact": (0, 1), "pi": (1,), "antiparallel": (0,), "orthogonal": (0,)}.get(kind, ())
            for i in exact:
                assert mine[b, i] == (ref_t, ref_R)[i], (b, kind, i)
            assert ref_t != ref_t or abs(mine[b, 0] - ref_t) < 1e-5 and abs(mine[b, 1] - ref_R) < 1e-5  # cosines next to 1
    print(f"restatement vs reference: worst pose error difference {worst:.3e} degrees over {seen} spread rows")
    assert seen >= 50 and worst <= POSE_ATOL_DEG


def test_pose_auc_restatement_matches_the_reference():
    g = cases.golden()
    worst = 0.0
    for name, e in cases.error_sets().items():
        o = cases.oracle()["summary"][name]
        pose = [o[cases.POSE_THRESHOLDS]["auc"][i] for i in (0, 1, 3)]  # 5, 10, 20 of 5, 10, 15, 20
        homog = o[cases.HOMOGRAPHY_THRESHOLDS]["auc"]
        ref_pose, ref_homog = g["ref_auc_pose_" + name], g["ref_auc_homog_" + name]
        if e.size == 0:
            # no error at all: 0 / 0 here and on the device; the reference's curve is then the origin alone and its area 0
            assert np.all(ref_pose == 0.0) and np.all(ref_homog == 0.0) and np.isnan(pose).all() and np.isnan(homog).all()
            continue
        bound = cases.auc_bound(e.size)
        assert rel_close(pose, ref_pose, bound) and rel_close(homog, ref_homog, bound), name
        for a, b in zip(pose + homog, list(ref_pose) + list(ref_homog)):
            if b != 0.0:
                worst = max(worst, abs(a - b) / abs(b) / bound)
    print(f"closed form vs reference pose_auc: worst relative difference at {worst:.2e} of (N + 8) 2^-52")


# --------------------------------------------------------------------------------------------------- the restatement itself
def test_degenerate_pose_rows_give_their_exact_values():
    p, o = cases.pose_cases(), cases.oracle()["pose"]
    by_kind = {k: o[p["kind"].index(k)] for k in cases.SPECIAL_KINDS}
    assert tuple(by_kind["same_exact"]) == (0.0, 0.0, 0.0)
    assert 0.0 <= by_kind["same_random"][0] < 1e-5 and 0.0 <= by_kind["same_random"][1] < 1e-5
    assert by_kind["pi"][1] == 180.0 and by_kind["pi"][2] == 180.0
    assert by_kind["antiparallel"][0] == 0.0 and by_kind["antiparallel"][1] < 1e-5
    assert by_kind["orthogonal"][0] == 90.0
    zt = by_kind["zero_t"]
    assert math.isnan(zt[0]) and zt[1] < 1e-5 and math.isnan(zt[2])  # Python's max(e_t, e_R) keeps a NaN e_t
    assert [tuple(o[b]) for b, k in enumerate(p["kind"]) if k == "not_ok"] == [(90.0, 90.0, 90.0)] * 2
    assert p["ok"].sum() == cases.N_POSE - 2 and np.isnan(p["R"][p["ok"] == 0]).any()
    spread = o[[k == "spread" for k in p["kind"]]]
    assert spread[:, 0].min() > 0.99 and spread[:, 0].max() <= 90.0 and spread[:, 1].min() > 0.99 and spread[:, 1].max() < 179.01
    assert np.array_equal(spread[:, 2], np.maximum(spread[:, 0], spread[:, 1]))


def test_corner_error_restatement_special_rows():
    c, o = cases.corner_cases(), cases.oracle()["corner"]
    row = {k: c["kind"].index(k) for k in ("same", "shift", "not_ok", "zero_row", "zero_left")}
    assert o[row["same"]] == 0.0
    side = min(c["sizes"][row["shift"]][2:])
    assert o[row["shift"]] == 5.0 / (side / 480.0)
    # the fallback matrix sends every corner to (0, 0): the mean norm of the true corners, whatever H_pred held
    b = row["not_ok"]
    w1, h1 = c["sizes"][b][:2]
    want = 0.0
    for x, y in ((0.0, 0.0), (0.0, h1 - 1), (w1 - 1, 0.0), (w1 - 1, h1 - 1)):
        q = c["Hg"][b] @ np.array([x, y, 1.0])
        want += math.hypot(q[0] / q[2], q[1] / q[2])
    assert abs(o[b] - want / 4 / (min(c["sizes"][b][2:]) / 480.0)) < 1e-9 and np.isfinite(o[[i for i, k in enumerate(c["kind"]) if k == "not_ok"]]).all()
    assert not np.isfinite(o[row["zero_row"]]) and not np.isfinite(o[row["zero_left"]])
    rnd = o[[k == "random" for k in c["kind"]]]
    assert np.isfinite(rnd).all() and 0.0 < np.median(rnd) < 100.0


def test_closed_form_auc_equals_sort_and_trapezoid_on_every_set():
    for name, e in cases.error_sets().items():
        for thr in (cases.POSE_THRESHOLDS, cases.HOMOGRAPHY_THRESHOLDS):
            s = cases.oracle()["summary"][name][thr]
            assert rel_close(s["auc"], mr.pose_auc_sorted(e, thr), cases.auc_bound(e.size)), (name, thr)
            assert s["n"] == e.size and s["below"] == [int((e < t).sum()) for t in thr]
            if e.size:
                assert s["acc"] == [float(np.float64(k) / np.float64(e.size)) for k in s["below"]]
                assert s["acc"] == [float((e < t).mean()) for t in thr]  # the benchmarks' accuracy lines
            else:
                assert np.isnan(s["acc"]).all() and np.isnan(s["auc"]).all()
    assert cases.oracle()["summary"]["none_below"][cases.POSE_THRESHOLDS]["auc"] == [0.0] * 4
    e = cases.error_sets()["n7500"]
    d = mr.pose_summary(e)
    acc = [(e < t).mean() for t in (5, 10, 15, 20)]
    assert d["map_5"] == acc[0] and d["map_10"] == np.mean(acc[:2]) and d["map_20"] == np.mean(acc)
    assert set(mr.homography_summary(e)) == {"hpatches_homog_auc_3", "hpatches_homog_auc_5", "hpatches_homog_auc_10"}


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [11, 10, 6, 11]
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "metrics.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "metrics" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()


def test_c_abi_validates_before_device_work(built_lib):
    import ctypes as C
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    thr = (C.c_double * 16)(*range(1, 17))

    def pose(*, R=p, t=p, T=p, rows=3, B=2, out=p, log=None, cap=0, state=None):
        return lib.roma_op_pose_error(R, t, None, T, rows, B, out, log, cap, state, None)
    for kw, word in ((dict(R=None), b"null"), (dict(t=None), b"null"), (dict(T=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=-1), b"B"), (dict(B=65536), b"B"), (dict(rows=2), b"t_rows"), (dict(rows=5), b"t_rows"),
                     (dict(R=20), b"aligned"), (dict(log=p), b"state"), (dict(state=p), b"state"), (dict(log=p, state=p, cap=0), b"capacity"),
                     (dict(log=20, state=p, cap=8), b"aligned")):
        assert pose(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    assert pose(B=0) == 0 and pose(B=0, log=p, state=p, cap=4) == 0  # nothing to do, nothing launched

    def corner(*, Hp=p, Hg=p, sizes=p, B=2, out=p, log=None, cap=0, state=None):
        return lib.roma_op_corner_error(Hp, None, Hg, sizes, B, out, log, cap, state, None)
    for kw, word in ((dict(Hp=None), b"null"), (dict(Hg=None), b"null"), (dict(sizes=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=65536), b"B"), (dict(sizes=12), b"aligned"), (dict(log=p), b"state"), (dict(log=p, state=p, cap=-1), b"capacity")):
        assert corner(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    assert corner(B=0) == 0

    def append(*, v=p, B=2, log=p, cap=8, state=p):
        return lib.roma_op_error_log_append(v, B, log, cap, state, None)
    for kw, word in ((dict(v=None), b"null"), (dict(log=None), b"null"), (dict(state=None), b"null"), (dict(B=65536), b"B"),
                     (dict(v=4), b"aligned"), (dict(cap=0), b"capacity")):
        assert append(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    assert append(B=0) == 0

    def summary(*, e=p, n=10, state=None, cap=0, t=thr, T=3, outs=(p, p, p, p)):
        return lib.roma_op_error_summary(e, n, state, cap, t, T, *outs, None)
    bad = (C.c_double * 3)(5.0, 0.0, 20.0)
    nan = (C.c_double * 3)(5.0, float("nan"), 20.0)
    inf = (C.c_double * 3)(5.0, float("inf"), 20.0)
    for kw, word in ((dict(e=None), b"null"), (dict(t=None), b"null"), (dict(outs=(p, None, p, p)), b"null"), (dict(T=0), b"[1, 16]"),
                     (dict(T=17), b"[1, 16]"), (dict(n=65537), b"65536"), (dict(n=-1), b"65536"), (dict(state=p, cap=65537), b"65536"),
                     (dict(state=p, cap=0), b"65536"), (dict(state=p, cap=8, e=None), b"null"), (dict(e=12), b"aligned"),
                     (dict(t=bad), b"positive"), (dict(t=nan), b"positive"), (dict(t=inf), b"positive")):
        assert summary(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())


def test_python_front_end_checks_arguments_and_refuses_host_tensors():
    import roma_amd
    from roma_amd import _lib
    for name in ("pose_error", "compute_pose_error", "homography_corner_error", "pose_auc", "ErrorLog", "ErrorSummary", "PoseError",
                 "hpatches_coordinates"):
        assert name in roma_amd.__all__ and callable(getattr(roma_amd, name))
    B = 4
    R, t, T = torch.eye(3).repeat(B, 1, 1), torch.ones(B, 3, 1), np.zeros((B, 3, 4))
    # shapes and dtypes, before the device is looked at (these are host tensors)
    for bad in (dict(R=torch.eye(4).repeat(B, 1, 1)), dict(R=torch.eye(3)), dict(t=torch.ones(B, 4)), dict(t=torch.ones(B + 1, 3)),
                dict(T_gt=np.zeros((B, 3, 3))), dict(T_gt=np.zeros((3, 4))), dict(T_gt=np.zeros((B + 1, 4, 4))),
                dict(R=torch.eye(3).repeat(B, 1, 1).int()), dict(ok=torch.ones(B)), dict(ok=torch.ones(B + 1, dtype=torch.bool)),
                dict(R=torch.zeros(65536, 3, 3), t=torch.zeros(65536, 3), T_gt=torch.zeros(65536, 3, 4))):
        with pytest.raises(ValueError):
            roma_amd.pose_error(**{**dict(R=R, t=t, T_gt=T), **bad})
    for bad in (dict(R=np.eye(3)), dict(log="log"), dict(log=torch.zeros(8))):
        with pytest.raises(TypeError):
            roma_amd.pose_error(**{**dict(R=R, t=t, T_gt=T), **bad})
    H, sizes = torch.eye(3).repeat(B, 1, 1), np.full((B, 4), 480.0)
    for bad in (dict(H_pred=torch.zeros(B, 3, 4)), dict(H_gt=np.zeros((B, 4, 3))), dict(H_gt=np.eye(3)), dict(sizes=np.zeros((B, 3))),
                dict(sizes=np.zeros(4)), dict(ok=torch.ones(B, dtype=torch.float32)), dict(sizes=np.zeros((B + 1, 4)))):
        with pytest.raises(ValueError):
            roma_amd.homography_corner_error(**{**dict(H_pred=H, H_gt=H.numpy(), sizes=sizes), **bad})
    with pytest.raises(TypeError):
        roma_amd.homography_corner_error(H.numpy(), H.numpy(), sizes)
    e = torch.zeros(10, dtype=torch.float64)
    for errors, thr in ((e, ()), (e, range(1, 18)), (e, (5.0, 0.0)), (e, (5.0, -1.0)), (e, (float("nan"),)), (e, (float("inf"),)),
                        (torch.zeros(2, 5), (5.0,)), (torch.zeros(10, dtype=torch.int64), (5.0,)), (torch.zeros(65537), (5.0,))):
        with pytest.raises(ValueError):
            roma_amd.pose_auc(errors, thr)
    with pytest.raises(TypeError):
        roma_amd.pose_auc(np.zeros(10), (5.0,))
    for cap in (0, -1, 65537):
        with pytest.raises(ValueError):
            roma_amd.ErrorLog(capacity=cap)
    log = roma_amd.ErrorLog.__new__(roma_amd.ErrorLog)  # the methods check their arguments before they look at the log
    for values in (torch.zeros(2, 3), torch.zeros(3, dtype=torch.int32), torch.zeros(65536)):
        with pytest.raises(ValueError):
            log.append(values)
    with pytest.raises(TypeError):
        log.append([1.0, 2.0])
    for thr in ((), (5.0, 0.0), tuple(range(1, 18))):
        with pytest.raises(ValueError):
            log.summary(thr)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        log.append(torch.zeros(3, dtype=torch.float64))
    # host tensors are refused: there is no CPU path
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.pose_error(R, t, T)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.pose_error(R[0], t[0], T[0])
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.compute_pose_error(T[0], R[0], t[0])
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.homography_corner_error(H, H.numpy(), sizes)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.pose_auc(e, (5.0, 10.0, 20.0))
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.ErrorLog(device="cpu")


def test_hpatches_coordinates_is_the_pixel_centre_convention():
    import roma_amd
    m = torch.tensor([[-1.0, -1.0, 1.0, 1.0], [0.0, 0.5, -0.25, 0.0]], dtype=torch.float64)
    a, b = roma_amd.hpatches_coordinates(m, 640, 480, 800, 600)
    assert a.tolist() == [[-0.5, -0.5], [319.5, 359.5]] and b.tolist() == [[799.5, 599.5], [299.5, 299.5]]
    ra, rb = mr.hpatches_coordinates(m.numpy(), 640, 480, 800, 600)
    assert np.array_equal(a.numpy(), ra) and np.array_equal(b.numpy(), rb)
    batch = torch.zeros(3, 7, 4)
    a, b = roma_amd.hpatches_coordinates(batch, 10, 20, 30, 40)
    assert a.shape == b.shape == (3, 7, 2) and a.dtype == torch.float32
    with pytest.raises(ValueError):
        roma_amd.hpatches_coordinates(torch.zeros(5, 2), 1, 1, 1, 1)


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_metrics_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "metrics.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/metrics.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["corner_error_kernel", "error_log_append_kernel", "error_summary_kernel", "pose_error_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
