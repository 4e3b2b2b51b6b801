"""tools/keypoints_ref.py (the oracle of roma_amd.match_keypoints, the batched form) against the reference's own match_keypoints
(tests/golden/keypoints_reference.npz, keypoints_ties_reference.npz) and against oracle.match_keypoints, the conditions
tests/test_gpu_keypoints_batched.py puts on the cases of tests/keypoints_cases.py, and the C ABI and Python surface of
roma_op_match_keypoints (dlopen only).  No GPU."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import keypoints_cases as cases

sys.path.insert(0, os.path.join(ROOT, "tools"))
import keypoints_ref as kr  # noqa: E402

NEW_SYMBOLS = ("roma_op_match_keypoints", "roma_op_match_keypoints_workspace")


# ------------------------------------------------------------------------------------------------- restatement against the reference
@pytest.mark.parametrize("params", list(cases.PARAMS))
@pytest.mark.parametrize("name, case", [("keypoints", 0), ("keypoints_ties", 1)])
def test_restatement_returns_the_reference_pairs(name, case, params):
    g = cases.golden(name)
    inds = kr.match_pair(g["x_A"], g["x_B"], g["warp"], g["cert"], **cases.PARAMS[params])[0]
    assert inds.dtype == np.int64 and np.array_equal(inds, cases.golden_inds(name, params))
    assert len(inds) == cases.PAIRS[case][params]
    assert np.array_equal(cases.expected(case, params), inds)


@pytest.mark.parametrize("params", list(cases.PARAMS))
@pytest.mark.parametrize("case", [2, 3, 4, 5, 6, "generated", "ties_matched"])
def test_restatement_agrees_with_the_oracle_and_no_case_is_a_near_tie(case, params):
    """keypoints_cases.checked asserts both; the figures are printed"""
    inds, gap, _, _ = cases.checked(case, params)
    print(f"case {case} ({params}): {len(inds)} pairs on {len(np.unique(inds[:, 0]))} rows of A, smallest relative gap {gap:.3g}")
    assert gap >= cases.MIN_GAP
    if case in cases.PAIRS:
        assert len(inds) == cases.PAIRS[case][params]
    if len(inds):  # row-major
        key = inds[:, 0] * (1 << 32) + inds[:, 1]
        assert np.all(np.diff(key) > 0)


def test_cases_take_every_path():
    sizes = [(len(p[0]), len(p[1])) for p in cases.pairs()]
    assert sizes == [(700, 900), (360, 517), (257, 511), (256, 512), (0, 333), (300, 0), (700, 900)]
    assert max(s[0] for s in sizes) == cases.NA and max(s[1] for s in sizes) == cases.NB
    flat = [v for s in sizes for v in s if v]
    assert any(v % 256 == 0 for v in flat) and any(v % 256 == 1 for v in flat) and any(v % 256 == 255 for v in flat)  # on and around a workgroup
    assert sum(v > 256 for v in flat) > 4  # more than one workgroup
    xa, xb, _, _ = cases.generated()
    assert xa.shape == (1300, 2) and xb.shape == (2100, 2) and xa.dtype == xb.dtype == np.float32
    assert len(xa) > 1024 and len(xb) > 2048 and len(xa) % 1024 and len(xb) % 1024  # a second and a third, partial LDS tile
    # the flipped warp is another warp: other pairs than pair 0, which has the same keypoints
    assert not np.array_equal(cases.expected(6, "loose"), cases.expected(0, "loose")) and len(cases.expected(6, "loose")) > 100
    # duplicate keypoints: more pairs than distinct rows, and in one case more pairs than rows of A at all
    for case in (1, "generated", "ties_matched"):
        inds = cases.expected(case, "default")
        assert len(inds) > len(np.unique(inds[:, 0]))
    assert len(cases.expected("ties_matched", "default")) > len(cases.ties_matched()[0])  # total > na
    # the cap case of the device test: max_matches below the total of both of its pairs
    assert min(len(cases.expected(c, "default")) for c in ("ties_matched", 0)) > CAP_M
    # both thresholds bite: the loose set drops pairs for certainty and the default set for distance
    assert len(cases.expected(0, "loose")) < len(cases.expected(0, "default")) and len(cases.expected(6, "loose")) > len(cases.expected(6, "default"))


CAP_M = 300  # max_matches of tests/test_gpu_keypoints_batched.py::test_max_matches_caps_the_rows_and_not_the_total


def test_batched_restatement_pads_counts_and_caps():
    b = cases.batch()
    assert b["x_A"].shape == (7, cases.NA, 2) and b["x_B"].shape == (7, cases.NB, 2) and b["warp"].shape == (7, 96, 128, 4)
    out = kr.match_keypoints(b["x_A"], b["x_B"], b["warp"], b["cert"], b["counts_A"], b["counts_B"])
    assert out["inds"].shape == (7, cases.NB, 2) and out["inds"].dtype == np.int32 and out["total"].dtype == np.int64
    for k in range(7):
        e = cases.expected(k, "default")
        n = len(e)
        assert out["total"][k] == out["counts"][k] == n
        assert np.array_equal(out["inds"][k, :n], e) and np.all(out["inds"][k, n:] == -1)
        assert np.array_equal(out["kpts_A"][k, :n], b["x_A"][k, e[:, 0]]) and np.all(out["kpts_A"][k, n:] == 0)
        assert np.array_equal(out["kpts_B"][k, :n], b["x_B"][k, e[:, 1]]) and np.all(out["kpts_B"][k, n:] == 0)
    # padding rows are not read: garbage there changes nothing
    nan = cases.batch(fill=np.nan)
    out_nan = kr.match_keypoints(nan["x_A"], nan["x_B"], nan["warp"], nan["cert"], nan["counts_A"], nan["counts_B"])
    assert all(np.array_equal(out[k], out_nan[k]) for k in out)
    # the cap, and pixel sizes
    cap = kr.match_keypoints(b["x_A"], b["x_B"], b["warp"], b["cert"], b["counts_A"], b["counts_B"], max_matches=CAP_M, sizes=(480, 640, 300, 400))
    assert cap["counts"][0] == CAP_M and cap["total"][0] == 478 and np.array_equal(cap["inds"][0], cases.expected(0, "default")[:CAP_M])
    assert cap["counts"][2] == 132 and np.all(cap["inds"][2, 132:] == -1)
    px = torch.from_numpy(b["x_A"][0, cases.expected(0, "default")[:CAP_M, 0]])
    assert np.array_equal(cap["kpts_A"][0], torch.stack((640 / 2 * (px[..., 0] + 1), 480 / 2 * (px[..., 1] + 1)), dim=-1).numpy())


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert len(_lib.SIGNATURES["roma_op_match_keypoints"][1]) == 28
    assert len(_lib.SIGNATURES["roma_op_match_keypoints_workspace"][1]) == 3
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "keypoints_batched.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "keypoints_batched" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()  # no packed f32 here
    assert "#define ROMA_ABI_VERSION" in header  # additive: the version is left alone (test_cpu_abi holds its value)


def workspace_formula(B, NA, NB):
    """include/roma_hip.h: p, c, the two arrays of minima and the int64 positions of (row, slice of B), each rounded up to 16 bytes;
    B is walked in at most 8 slices of whole 1024-point tiles, as many as bring the count kernel to 1024 workgroups"""
    r16 = lambda n: (n + 15) // 16 * 16  # noqa: E731
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    want = max(1, min(max(1, cdiv(NB, 1024)), 8, cdiv(1024, B * max(1, cdiv(NA, 256)))))
    per = max(1024, cdiv(cdiv(NB, want), 1024) * 1024)
    slices = max(1, cdiv(NB, per))
    return r16(B * NA * 8) + 2 * r16(B * NA * 4) + r16(B * NB * 4) + r16(B * NA * slices * 8)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_workspace_formula(built_lib, fmt):
    from roma_amd import _lib
    lib = _lib.load(fmt)
    assert lib.roma_op_match_keypoints_workspace(1, 1, 1) == 16 * 5
    assert lib.roma_op_match_keypoints_workspace(8, 4096, 4096) == 8 * 4096 * (8 + 4 + 4 + 4 + 4 * 8)  # 4 slices of 1024
    assert lib.roma_op_match_keypoints_workspace(3, 0, 0) == 0
    for shape in ((1, 1, 1), (7, 700, 900), (1, 1300, 2100), (8, 4096, 4096), (8, 8192, 8192), (1, 8192, 8192), (2, 0, 5), (2, 5, 0),
                  (65535, 3, 2), (1, 1 << 20, 1 << 20), (64, 300, 20000), (1, 257, 9000)):
        assert lib.roma_op_match_keypoints_workspace(*shape) == workspace_formula(*shape), shape
    for bad in ((0, 5, 5), (65536, 5, 5), (1, -1, 5), (1, 5, -1), (1, (1 << 20) + 1, 5), (1, 5, (1 << 20) + 1)):
        assert lib.roma_op_match_keypoints_workspace(*bad) == -1


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_c_abi_validates_before_device_work(built_lib, fmt):
    from roma_amd import _lib
    lib = _lib.load(fmt)
    B, NA, NB, H, W, M = 3, 700, 900, 96, 128, 900
    # addresses that are never used: validation must fail first.  Aligned as their types ask.
    XA, XB, CA, CB, WARP, CERT, SZ, INDS, KA, KB, CNT, TOT, WS = (k << 20 for k in range(1, 14))
    need = lib.roma_op_match_keypoints_workspace(B, NA, NB)
    assert need == workspace_formula(B, NA, NB)

    def call(*, xa=XA, xb=XB, ca=CA, cb=CB, warp=WARP, sb=H * W * 4, sr=W * 4, cert=CERT, tb=H * W, tr=W, sz=None, ss=0, B=B, NA=NA, NB=NB,
             H=H, W=W, max_dist=0.005, cert_th=0.0, M=M, inds=INDS, ka=KA, kb=KB, cnt=CNT, tot=TOT, ws=WS, ws_bytes=need):
        return lib.roma_op_match_keypoints(xa, xb, ca, cb, warp, sb, sr, cert, tb, tr, sz, ss, B, NA, NB, H, W, max_dist, cert_th, M, inds, ka,
                                           kb, cnt, tot, ws, ws_bytes, None)
    for kw, word in ((dict(xa=None), b"null"), (dict(xb=None), b"null"), (dict(warp=None), b"null"), (dict(cert=None), b"null"),
                     (dict(inds=None), b"null"), (dict(ka=None), b"null"), (dict(kb=None), b"null"), (dict(cnt=None), b"null"),
                     (dict(tot=None), b"null"), (dict(ws=None), b"null"), (dict(B=0), b"B must"), (dict(B=65536), b"B must"),
                     (dict(NA=-1), b"NA and NB"), (dict(NB=-1), b"NA and NB"), (dict(NA=(1 << 20) + 1), b"NA and NB"),
                     (dict(NB=(1 << 20) + 1), b"NA and NB"), (dict(M=0), b"max_matches"), (dict(M=-5), b"max_matches"),
                     (dict(M=1 << 31), b"max_matches"), (dict(H=0), b"warp grid"), (dict(W=0), b"warp grid"), (dict(W=-3), b"warp grid"),
                     (dict(sr=W * 4 - 4), b"warp strides"), (dict(sr=W * 4 + 2), b"warp strides"), (dict(sb=(H - 1) * W * 4), b"warp strides"),
                     (dict(sb=H * W * 4 + 1), b"warp strides"), (dict(tr=W - 1), b"certainty strides"), (dict(tb=H * W - 1), b"certainty strides"),
                     (dict(sz=SZ, ss=3), b"sizes stride"), (dict(sz=SZ, ss=-4), b"sizes stride"), (dict(warp=WARP + 8), b"16-byte"),
                     (dict(ws=WS + 4), b"16-byte"), (dict(xa=XA + 2), b"aligned"), (dict(xb=XB + 1), b"aligned"), (dict(ca=CA + 2), b"aligned"),
                     (dict(cb=CB + 2), b"aligned"), (dict(cert=CERT + 2), b"aligned"), (dict(sz=SZ + 2), b"aligned"),
                     (dict(inds=INDS + 2), b"aligned"), (dict(ka=KA + 2), b"aligned"), (dict(kb=KB + 2), b"aligned"),
                     (dict(cnt=CNT + 2), b"aligned"), (dict(tot=TOT + 4), b"aligned"), (dict(max_dist=float("nan")), b"NaN"),
                     (dict(cert_th=float("nan")), b"NaN"), (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert call(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    # optional pointers, empty sides and infinite thresholds are valid: these pass every check but the last, the workspace size
    for kw in (dict(ca=None, cb=None), dict(sz=SZ, ss=0), dict(sz=SZ, ss=4), dict(NA=0, xa=None), dict(NB=0, xb=None), dict(NA=0, NB=0, xa=None, xb=None),
               dict(max_dist=float("inf"), cert_th=float("-inf")), dict(B=65535), dict(NA=1 << 20, NB=1 << 20), dict(M=1), dict(M=(1 << 31) - 1),
               dict(sr=W * 8, sb=H * W * 8, tr=2 * W, tb=2 * H * W)):
        assert call(**{**kw, "ws_bytes": -1}) != 0 and b"workspace is too small" in lib.roma_last_error(), (kw, lib.roma_last_error())


def _host_args():
    return dict(x_A=torch.zeros(2, 5, 2), x_B=torch.zeros(2, 7, 2), warp=torch.zeros(2, 4, 6, 4), certainty=torch.zeros(2, 4, 6))


def test_python_front_end_checks_arguments_and_refuses_host_tensors():
    import roma_amd
    from roma_amd import _lib
    from roma_amd.matcher import RegressionMatcher
    assert "match_keypoints" in roma_amd.__all__ and "KeypointMatches" in roma_amd.__all__ and callable(roma_amd.match_keypoints)
    assert roma_amd.KeypointMatches._fields == ("kpts_A", "kpts_B", "inds", "counts", "total")
    assert callable(RegressionMatcher.match_keypoints_batched)
    doc = roma_amd.match_keypoints.__doc__
    assert "model.match(" in doc and "match_keypoints(" in doc and "sizes=" in doc and "find_fundamental(" in doc and "counts=m.counts" in doc
    a = _host_args()
    # shapes, dtypes and values, before the device is looked at (these are host tensors)
    for bad in (dict(x_A=torch.zeros(2, 5, 3)), dict(x_A=torch.zeros(2, 5, 2, dtype=torch.int32)), dict(x_B=torch.zeros(7, 2)),
                dict(x_B=torch.zeros(3, 7, 2)), dict(x_A=torch.zeros(0, 5, 2), x_B=torch.zeros(0, 7, 2), warp=torch.zeros(0, 4, 6, 4)),
                dict(warp=torch.zeros(2, 4, 6, 2)), dict(warp=torch.zeros(2, 4, 6, 4, dtype=torch.float64)), dict(warp=torch.zeros(4, 6, 4)),
                dict(warp=torch.zeros(2, 0, 6, 4)), dict(warp=torch.zeros(3, 4, 6, 4), certainty=torch.zeros(3, 4, 6)),
                dict(certainty=torch.zeros(2, 4, 7)), dict(certainty=torch.zeros(2, 4, 6, dtype=torch.float64)),
                dict(warp=torch.zeros(2, 4, 7, 4), certainty=torch.zeros(2, 4, 7), symmetric=True),
                dict(counts_A=torch.zeros(3, dtype=torch.int32)), dict(counts_B=torch.zeros(2)), dict(counts_B=torch.zeros(2, 1, dtype=torch.int64)),
                dict(max_matches=0), dict(max_matches=1 << 31), dict(max_dist=float("nan")), dict(cert_th=float("nan")),
                dict(sizes=(480, 640, 480)), dict(sizes=(480, 640, 480, 0)), dict(sizes=(480, 640, float("inf"), 3)),
                dict(sizes=torch.ones(3, 4)), dict(sizes=torch.ones(2, 3))):
        kw = {**a, **bad}
        with pytest.raises(ValueError):
            roma_amd.match_keypoints(kw.pop("x_A"), kw.pop("x_B"), kw.pop("warp"), kw.pop("certainty"), **kw)
    with pytest.raises(ValueError):  # counts belong to the batched form
        roma_amd.match_keypoints(a["x_A"][0], a["x_B"][0], a["warp"][0], a["certainty"][0], counts_A=torch.zeros(1, dtype=torch.int32))
    for bad in (dict(x_A=np.zeros((2, 5, 2), np.float32)), dict(warp=None), dict(counts_A=[5, 5]), dict(sizes=640)):
        kw = {**a, **bad}
        with pytest.raises(TypeError):
            roma_amd.match_keypoints(kw.pop("x_A"), kw.pop("x_B"), kw.pop("warp"), kw.pop("certainty"), **kw)
    # host tensors are refused: there is no CPU path
    i32 = torch.full((2,), 3, dtype=torch.int32)
    calls = (lambda: roma_amd.match_keypoints(a["x_A"], a["x_B"], a["warp"], a["certainty"]),
             lambda: roma_amd.match_keypoints(a["x_A"][0], a["x_B"][0], a["warp"][0], a["certainty"][0], sizes=(4, 6, 4, 6)),
             lambda: roma_amd.match_keypoints(a["x_A"], a["x_B"], a["warp"], a["certainty"], i32, i32.long(), max_matches=3, symmetric=True,
                                              sizes=torch.ones(2, 4)),
             lambda: RegressionMatcher.__new__(RegressionMatcher).match_keypoints_batched(a["x_A"], a["x_B"], a["warp"], a["certainty"], i32, i32,
                                                                                         max_dist=0.02, cert_th=0.6))
    for fn in calls:
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            fn()


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_keypoint_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "keypoints_batched.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/keypoints_batched.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["kp_nn_kernel", "kp_pairs_kernel<0>", "kp_pairs_kernel<1>", "kp_sample_kernel", "kp_scan_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
