"""tools/gt_warp_ref.py (the oracle of roma_amd.warp_kpts / get_gt_warp / dense_metrics) against what the unmodified reference
returned on the scene of tests/gt_warp_cases.py (tests/golden/gt_warp_reference.npz), the conditions tests/test_gpu_gt_warp.py puts
on that scene, and the C ABI and Python surface of roma_op_warp_kpts / roma_op_dense_metrics (dlopen only).  No GPU."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import gt_warp_cases as cases

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gt_warp_ref as gw  # noqa: E402

NEW_SYMBOLS = ("roma_op_warp_kpts", "roma_op_dense_metrics_workspace", "roma_op_dense_metrics")
# oracle against reference: the two differ only in how the 3 x 3 inverse and the matrix products round (LU and FMA in torch's BLAS,
# the written order here): cond(K) ~ 1e3 and coordinates <= 1e3 give ~1e-10
ATOL = 1e-9


def same_nonfinite(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and \
        np.array_equal(np.isneginf(a), np.isneginf(b))


# ------------------------------------------------------------------------------------------------- oracle against the golden
def test_recorded_scene_is_the_generated_one():
    """the golden holds the bits the reference ran on; the generator reproduces them up to this machine's libm"""
    built, s = cases.build_scene(), cases.scene()
    for k in cases.INPUTS:
        assert built[k].shape == s[k].shape and built[k].dtype == s[k].dtype, k
        tol = 1e-6 if k == "matches" else 1e-12  # matches: float32 of (warp + noise), one ulp where the warp moves by 1e-16
        assert np.allclose(built[k], s[k], rtol=tol, atol=tol, equal_nan=True), k
    assert s["kpts"].shape == (cases.B, cases.L, 2) and s["kpts"].dtype == np.float32 and cases.L == 1003
    assert s["depth0"].shape == (cases.B, 23, 31) and s["depth1"].shape == (cases.B, 19, 37)


def test_warp_kpts_oracle_matches_the_reference():
    g, o = cases.golden(), cases.oracle()
    worst_w, worst_r = 0.0, 0.0
    for b in range(cases.B):
        w = o["warp"][b]
        assert np.array_equal(w["valid"], g["ref_valid"][b]), b  # every row
        ref_w, ref_r = g["ref_warped"][b], g["ref_rel"][b]
        assert same_nonfinite(w["warped"], ref_w) and same_nonfinite(w["rel"], ref_r), b
        fw = np.isfinite(ref_w)
        dw = np.abs(w["warped"] - ref_w) * [cases.W1 / 2, cases.H1 / 2]  # pixels of image 1
        fr = np.isfinite(ref_r)
        dr = np.abs(w["rel"][fr] - ref_r[fr])
        worst_w, worst_r = max(worst_w, dw[fw].max()), max(worst_r, dr.max())
    print(f"oracle vs reference: worst |warped| difference {worst_w:.3e} px, worst |rel| difference {worst_r:.3e}")
    assert worst_w <= ATOL and worst_r <= ATOL


def test_dense_metrics_oracle_matches_the_reference():
    g, o = cases.golden(), cases.oracle()
    m = o["metrics"]
    for b in range(cases.B):
        assert np.array_equal(m[b]["prob"], g["ref_prob"][b]), b
    gd = np.concatenate([m[b]["gd"][m[b]["prob"] == 1] for b in range(cases.B)])  # the reference's gd[prob == 1], batch-major
    ref_gd = g["ref_gd"]
    assert gd.shape == ref_gd.shape
    worst = np.abs(gd - ref_gd).max()
    print(f"oracle vs reference: worst |gd| difference {worst:.3e} px over {gd.size} valid pixels")
    assert worst <= ATOL
    epe, pck, n, total = cases.batch_means(m)
    assert n == ref_gd.size == sum(mm["n_valid"] for mm in m)
    # PCK counts: the reference reports float32 means of 0 / 1 over n pixels
    for k, thr in enumerate(cases.PCK):
        count = int((ref_gd < thr).sum())
        assert int(sum(mm["n_below"][k] for mm in m)) == count
        assert abs(pck[k] - count / n) < 1e-15 and abs(g["ref_pck"][k] - count / n) < 2.0 ** -23
    # any summation order of n terms: n 2^-52 sum |gd|, for both sides
    bound = n * 2.0 ** -52 * ref_gd.sum()
    print(f"oracle vs reference: EPE {epe:.6f} px, difference {abs(epe - ref_gd.mean()):.3e} (bound {bound:.3e}); PCK {pck}")
    assert abs(epe - ref_gd.mean()) <= bound and abs(total - ref_gd.sum()) <= bound


def test_grid_is_the_rounded_value_of_the_reference_linspace():
    """The reference builds its grid with a float32 linspace(-1 + 1/n, 1 - 1/n, n), which rounds start, step and start + j step in
    the binade of its end points, [0.5, 1): its error is one float32 ulp there, 2^-24, also where the value itself is small (the
    centre of an odd grid is exactly 0 here and -7.5e-9 there).  The oracle's grid - float32 of the float64 value - lies within that
    ulp of the reference's, element by element, and is the correctly rounded value wherever they differ."""
    g = cases.golden()
    x1 = g["ref_gt_x1_n"]
    assert x1.shape == (cases.B, cases.H0 * cases.W0, 2) and x1.dtype == np.float64
    mine = gw.grid(cases.H0, cases.W0)
    assert mine.dtype == np.float32
    ulp = np.maximum(np.spacing(np.abs(mine)).astype(np.float64), 2.0 ** -24)
    exact = np.stack(np.meshgrid((2 * np.arange(cases.W0) + 1) / cases.W0 - 1, (2 * np.arange(cases.H0) + 1) / cases.H0 - 1), axis=-1)
    exact = exact.reshape(-1, 2)
    for b in range(cases.B):
        assert np.all(np.abs(mine.astype(np.float64) - x1[b]) <= ulp)
        assert np.all(np.abs(mine.astype(np.float64) - exact) <= np.abs(x1[b] - exact) + 1e-17)
    print(f"grid: {float((mine.astype(np.float64) == x1[0]).mean()):.3f} of the values equal the reference's bit for bit")


def test_get_gt_warp_oracle_on_the_reference_grid_matches_the_reference():
    g, s = cases.golden(), cases.scene()
    worst = 0.0
    for b in range(cases.B):
        o = gw.warp_kpts(g["ref_gt_x1_n"][b], s["depth0"][b], s["depth1"][b], s["T"][b], s["K0"][b], s["K1"][b], cases.THRESHOLD)
        ref_x2 = g["ref_gt_x2"][b].reshape(-1, 2)
        assert np.array_equal(o["valid"].astype(np.float32), g["ref_gt_prob"][b].reshape(-1)), b
        assert same_nonfinite(o["warped"], ref_x2)
        f = np.isfinite(ref_x2)
        worst = max(worst, (np.abs(o["warped"] - ref_x2) * [cases.W1 / 2, cases.H1 / 2])[f].max())
    print(f"get_gt_warp: oracle on the reference's grid, worst difference {worst:.3e} px")
    assert worst <= ATOL


# --------------------------------------------------------------------------------------------------------- scene conditions
def test_scene_has_no_near_rows_and_shows_every_population():
    """what tests/test_gpu_gt_warp.py relies on: no deciding quantity within 1e-9 relative of its threshold (such a row could fall
    either way on the device), and every branch of the rule is taken by some row"""
    o = cases.oracle()
    seen = {k: 0 for k in ("valid", "zero", "not_covisible", "inconsistent", "inf", "nan", "outside")}
    s = cases.scene()
    for b in range(cases.B):
        w = o["warp"][b]
        assert not w["near"].any() and not o["gt"][b][2].any() and not o["gt_grid"][b][2].any() and not o["metrics"][b]["near"].any(), b
        seen["valid"] += int(w["valid"].sum())
        seen["zero"] += int((~w["nonzero"]).sum())
        seen["not_covisible"] += int((w["nonzero"] & ~w["covisible"]).sum())
        seen["inconsistent"] += int((w["nonzero"] & w["covisible"] & ~w["consistent"] & np.isfinite(w["rel"])).sum())
        seen["inf"] += int(np.isinf(w["rel"]).sum())
        seen["nan"] += int(np.isnan(w["rel"]).sum())
        seen["outside"] += int((np.abs(s["kpts"][b]) > 1).any(axis=1).sum())
        assert o["metrics"][b]["n_valid"] > 100 and 0 < o["metrics"][b]["n_below"][0] < o["metrics"][b]["n_below"][1], b
    print("rows per population:", seen)
    assert all(v > 0 for v in seen.values()), seen
    # pair 3: the zero block of depth0 projects through the bare 1e-4 and lands far outside
    w3 = o["warp"][3]
    assert np.isnan(w3["rel"]).sum() == (~w3["nonzero"]).sum() > 0 and np.abs(w3["u"][~w3["nonzero"]]).min() > 1e4
    assert all(np.isnan(o["warp"][b]["rel"]).sum() == 0 for b in range(3))


def test_sampling_rule_at_the_edges_and_for_non_finite_coordinates():
    D = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    nx = lambda px: 2.0 * (px + 0.5) / 4 - 1.0  # noqa: E731  normalised x of pixel-centre index px
    ny = lambda py: 2.0 * (py + 0.5) / 3 - 1.0  # noqa: E731
    x = np.array([nx(1), nx(0.5), nx(-0.5), nx(3.5), nx(-1.0), 1e7, np.inf, np.nan, nx(2)])
    y = np.array([ny(1), ny(1), ny(0), ny(2.5), ny(0), ny(1), ny(1), ny(1), -np.inf])
    v = gw.sample(D, x, y)
    assert np.allclose(v, [6.0, 5.5, 0.5, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0], rtol=0, atol=1e-14) and np.all(v[4:] == 0.0), v
    ref = torch.nn.functional.grid_sample(torch.from_numpy(D).double()[None, None], torch.from_numpy(np.stack([x, y], -1))[None, None],
                                          mode="bilinear", align_corners=False)[0, 0, 0].numpy()
    assert np.allclose(v[:6], ref[:6], atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert len(_lib.SIGNATURES["roma_op_warp_kpts"][1]) == 22
    assert len(_lib.SIGNATURES["roma_op_dense_metrics"][1]) == 30
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "gt_warp.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "gt_warp" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()  # no packed f32 here


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null 16-byte aligned address: validation must fail before it is used

    def warp(*, kpts=p, f64=0, grid=(0, 0), d0=p, d1=p, T=p, rows=3, K0=p, K1=p, B=2, L=1000, sizes=(23, 31, 19, 37), thr=0.05, out=p):
        return lib.roma_op_warp_kpts(kpts, f64, *grid, d0, d1, T, rows, K0, K1, B, L, *sizes, thr, None, None, None, out, None)
    for kw, word in ((dict(d0=None), b"null"), (dict(d1=None), b"null"), (dict(T=None), b"null"), (dict(K0=None), b"null"),
                     (dict(K1=None), b"null"), (dict(out=None), b"null"), (dict(B=-1), b"B"), (dict(B=65536), b"B"),
                     (dict(L=-3), b"negative"), (dict(B=2, L=1 << 30), b"2^31"), (dict(rows=2), b"t_rows"), (dict(rows=5), b"t_rows"),
                     (dict(f64=2), b"kpts_f64"), (dict(sizes=(0, 31, 19, 37)), b"sizes"), (dict(sizes=(23, 31, 19, 32769)), b"sizes"),
                     (dict(kpts=None, grid=(0, 31), L=0), b"grid"), (dict(kpts=None, grid=(10, 100), L=999), b"grid"),
                     (dict(kpts=None, grid=(32769, 1), L=32769), b"grid"), (dict(kpts=20, f64=1), b"aligned"),
                     (dict(kpts=18, f64=0), b"aligned"), (dict(thr=-0.1), b"negative"), (dict(thr=float("nan")), b"negative")):
        assert warp(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    for kw in (dict(B=0), dict(L=0), dict(kpts=None, grid=(10, 100), B=0)):
        assert warp(**kw) == 0  # nothing to do, nothing launched

    def met(*, m=p, sb=17 * 29 * 4, sr=29 * 4, d1=p, d2=p, T=p, rows=3, K1=p, K2=p, B=2, h=17, w=29, sizes=(23, 31, 19, 37), thr=0.05,
            pck=(1.0, 3.0, 5.0), outs=(p, p, p, p, p), ws=p, ws_bytes=1 << 20):
        return lib.roma_op_dense_metrics(m, sb, sr, d1, d2, T, rows, K1, K2, B, h, w, *sizes, thr, *pck, *outs, None, None, ws, ws_bytes,
                                         None)
    for kw, word in ((dict(m=None), b"null"), (dict(d1=None), b"null"), (dict(d2=None), b"null"), (dict(T=None), b"null"),
                     (dict(K1=None), b"null"), (dict(K2=None), b"null"), (dict(outs=(p, p, None, p, p)), b"null"), (dict(ws=None), b"null"),
                     (dict(B=0), b"B"), (dict(B=65536), b"B"), (dict(h=0), b"grid"), (dict(w=32769, sr=4 * 32769), b"grid"),
                     (dict(B=4, h=32768, w=32768, sr=4 * 32768, sb=4 << 30), b"2^31"), (dict(rows=6), b"t_rows"),
                     (dict(sizes=(23, 31, 0, 37)), b"sizes"), (dict(sr=29 * 4 - 4), b"strides"), (dict(sr=29 * 4 + 2), b"strides"),
                     (dict(sb=16 * 29 * 4), b"strides"), (dict(m=24), b"aligned"), (dict(ws=20), b"aligned"), (dict(thr=-1.0), b"negative"),
                     (dict(pck=(1.0, -3.0, 5.0)), b"negative"), (dict(ws_bytes=8), b"workspace")):
        assert met(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    # the workspace: 40 bytes per workgroup, whose number per pair does not depend on B
    one = lib.roma_op_dense_metrics_workspace(1, 17, 29)
    assert one == 2 * 40 and lib.roma_op_dense_metrics_workspace(4, 17, 29) == 4 * one
    assert lib.roma_op_dense_metrics_workspace(8, 560, 560) == 8 * 256 * 40
    assert lib.roma_op_dense_metrics_workspace(-1, 17, 29) == -1 and lib.roma_op_dense_metrics_workspace(1, 32769, 2) == -1


def _host_args(B=2, L=10):
    return dict(kpts0=torch.zeros(B, L, 2), depth0=torch.ones(B, 5, 6), depth1=torch.ones(B, 4, 7), T_0to1=np.zeros((B, 3, 4)),
                K0=np.stack([np.eye(3)] * B), K1=np.stack([np.eye(3)] * B))


def test_python_front_end_checks_arguments_and_refuses_host_tensors():
    import roma_amd
    from roma_amd import _lib
    from roma_amd.matcher import RegressionMatcher
    for name in ("warp_kpts", "get_gt_warp", "dense_metrics"):
        assert name in roma_amd.__all__ and callable(getattr(roma_amd, name))
    assert callable(RegressionMatcher.dense_metrics)
    a = _host_args()
    # unsupported modes, before anything else
    with pytest.raises(NotImplementedError, match="grid_sample"):
        roma_amd.warp_kpts(**a, depth_interpolation_mode="combined")
    with pytest.raises(NotImplementedError, match="grid_sample"):
        roma_amd.warp_kpts(**a, depth_interpolation_mode="nearest-exact")
    with pytest.raises(NotImplementedError, match="smooth_mask"):
        roma_amd.warp_kpts(**a, smooth_mask=0.1)
    with pytest.raises(NotImplementedError, match="grid_sample"):
        roma_amd.get_gt_warp(a["depth0"], a["depth1"], a["T_0to1"], a["K0"], a["K1"], depth_interpolation_mode="combined")
    with pytest.raises(ValueError, match="bilinear"):
        roma_amd.warp_kpts(**a, depth_interpolation_mode="bicubic")
    # shapes and dtypes, before the device is looked at (these are host tensors)
    for bad in (dict(kpts0=torch.zeros(2, 10, 3)), dict(kpts0=torch.zeros(2, 10, 2, dtype=torch.float16)), dict(kpts0=torch.zeros(10, 2)),
                dict(depth0=torch.ones(2, 5, 6, dtype=torch.float64)), dict(depth0=torch.ones(3, 5, 6)), dict(depth1=torch.ones(2, 4)),
                dict(depth1=torch.ones(1, 4, 7)), dict(T_0to1=np.zeros((2, 3, 3))), dict(T_0to1=np.zeros((3, 4))),
                dict(K0=np.eye(3)), dict(K1=np.zeros((2, 3, 4))), dict(relative_depth_error_threshold=-0.1)):
        with pytest.raises(ValueError):
            roma_amd.warp_kpts(**{**a, **bad})
    with pytest.raises(TypeError):
        roma_amd.warp_kpts(**{**a, "kpts0": np.zeros((2, 10, 2))})
    g = (a["depth0"], a["depth1"], a["T_0to1"], a["K0"], a["K1"])
    for kw in (dict(H=4), dict(H=0, W=3), dict(H=40000, W=3)):
        with pytest.raises(ValueError):
            roma_amd.get_gt_warp(*g, **kw)
    m = torch.zeros(2, 3, 4, 4)
    for bad_m in (torch.zeros(2, 3, 4, 2), torch.zeros(2, 3, 4, 4, dtype=torch.float64), torch.zeros(3, 4, 4), torch.zeros(3, 3, 4, 4)):
        with pytest.raises(ValueError):
            roma_amd.dense_metrics(bad_m, *g)
    for kw in (dict(thresholds=(1.0, 3.0)), dict(thresholds=(1.0, -3.0, 5.0)), dict(relative_depth_error_threshold=float("nan"))):
        with pytest.raises(ValueError):
            roma_amd.dense_metrics(m, *g, **kw)
    # host tensors are refused: there is no CPU path
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.warp_kpts(**a)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.warp_kpts(**a, return_relative_depth_error=True)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.get_gt_warp(*g)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.get_gt_warp(*g, H=3, W=4)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.dense_metrics(m, *g)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        RegressionMatcher.__new__(RegressionMatcher).dense_metrics(m, *g, return_maps=True)


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_gt_warp_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "gt_warp.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/gt_warp.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["dense_metrics_finish_kernel", "dense_metrics_kernel", "warp_kpts_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
