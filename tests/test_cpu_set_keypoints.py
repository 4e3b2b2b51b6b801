"""The numpy oracle of the detector-free keypoints - tools/set_keypoints_ref.py against a hand-made case whose expected output is
written out, the property its one-pass suppression guarantees, its invariances, and the conditions the chain on a scene must meet -
and the C ABI and Python surface of roma_op_keypoints_from_matches without a GPU (argument validation only)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from set_keypoints_cases import (RANDOM_SIZES, check_hand_made, hand_made, random_case, ref, scene_case, scene_tracks, skr)

NEW_SYMBOLS = ["roma_op_keypoints_from_matches", "roma_op_keypoints_from_matches_workspace"]
KERNELS = ["skp_assign_kernel", "skp_clear_kernel", "skp_finish_kernel", "skp_number_kernel", "skp_scan_kernel", "skp_scatter_kernel",
           "skp_suppress_kernel"]


@pytest.mark.parametrize("radius", [2.0, 0.0])
def test_ref_on_the_hand_made_case(radius):
    check_hand_made(ref(hand_made(), cell=2, radius=radius, max_kpts=8), radius)


def test_fma_sq_rounds_once():
    """fl32(dy dy + fl32(dx dx)) against exact rational arithmetic, on values whose float64 sum is inexact"""
    from fractions import Fraction
    g = np.random.default_rng(0)
    dy = (g.uniform(-3, 3, 4000) * 2.0 ** g.integers(-12, 8, 4000)).astype(np.float32)
    dx = (g.uniform(-3, 3, 4000) * 2.0 ** g.integers(-12, 8, 4000)).astype(np.float32)
    got = skr.fma_sq(dy, dx)
    for a, b, r in zip(dy, dx, got):
        exact = Fraction(float(a)) ** 2 + Fraction(float(np.float32(b * b)))
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        assert abs(Fraction(float(r)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


@pytest.mark.parametrize("cell,radius", [(1, 1.0), (2, 1.0), (2, 2.0), (3, 3.0), (3, 1.5)])
def test_no_two_keypoints_of_neighbouring_cells_lie_within_the_radius(cell, radius):
    """What the one-pass rule guarantees: of two candidates in 8-neighbouring cells with d2 <= radius^2 the one with the smaller
    key never survives (a suppressed candidate still suppresses), so no two KEPT keypoints of a view in neighbouring cells have
    d2 <= radius^2 - in the operator's own d2, exactly.  Keypoints of cells that are not neighbours are more than a cell, hence
    more than the radius, apart.  (The rule does not promise the converse: a candidate may go although what suppressed it went
    too.)"""
    c = random_case(0)
    o = ref(c, cell=cell, radius=radius, max_kpts=4096)
    r2 = np.float32(radius) * np.float32(radius)
    assert o["info"][5] > 0
    for v, (H, W) in enumerate(RANDOM_SIZES):
        n = int(o["num_kpts"][v])
        x, y = o["kpts"][v, :n, 0], o["kpts"][v, :n, 1]
        cx, cy = np.floor(x).astype(int) // cell, np.floor(y).astype(int) // cell
        assert np.array_equal(np.sort(cy * ((W + cell - 1) // cell) + cx), cy * ((W + cell - 1) // cell) + cx)  # ascending cell id
        d2 = skr.fma_sq(y[:, None] - y[None, :], x[:, None] - x[None, :])
        near = (np.abs(cx[:, None] - cx[None, :]) <= 1) & (np.abs(cy[:, None] - cy[None, :]) <= 1) & ~np.eye(n, dtype=bool)
        assert near.any() and (d2[near] > r2).all()
        far = ~near & ~np.eye(n, dtype=bool)
        assert (np.hypot(x[:, None] - x[None, :], y[:, None] - y[None, :])[far] > cell).all()


def test_result_does_not_change_when_invalid_rows_are_appended():
    c = random_case(0)
    P, N = c["certainty"].shape
    extra = 5
    m = np.zeros((P, N + extra, 4), np.float32)
    cert = np.zeros((P, N + extra), np.float32)
    bad = [((np.nan, 0, 0, 0), 1.0), ((0, 0, 0, 0), 0.0), ((1.0, 0, 0, 0), 1.0), ((0, 0, 0, -1.5), 1.0), ((0, 0, 0, 0), np.inf)]
    for p in range(P):
        k = int(c["counts"][p])
        m[p, :k], cert[p, :k] = c["matches"][p, :k], c["certainty"][p, :k]
        for i, (row, cc) in enumerate(bad):
            m[p, k + i], cert[p, k + i] = row, cc
    d = dict(c, matches=m, certainty=cert, counts=c["counts"] + extra)
    for kw in (dict(cell=2, max_kpts=4096), dict(cell=1, radius=0.5, max_kpts=100), dict(cell=3, radius=0.0, max_kpts=4096, one_to_one=False)):
        a, b = ref(c, **kw), ref(d, **kw)
        for key in ("kpts", "score", "num_kpts", "total", "kept"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        for p in range(P):
            k = int(c["counts"][p])
            assert np.array_equal(a["inds"][p, :k], b["inds"][p, :k]) and (b["inds"][p, k:] == -1).all() and (a["inds"][p, k:] == -1).all()
        assert b["info"] == (a["info"][0] + extra * P, a["info"][1] + extra * P) + a["info"][2:]


def test_chain_conditions_hold_on_the_restatement():
    """the scene's pairwise matches, jittered by +-0.25 px per endpoint: tracks >= 90 % of the points seen in two views or more
    and components dropped <= 5 % of them with the suppression stage; fewer than 75 % without it.  Measured: 290 of 292 tracks
    (99.3 %) and 1 component dropped (0.3 %) at radius = cell = 2; 173 tracks (59.2 %) at radius 0."""
    case, scene = scene_case()
    n = scene["seen2"]
    on = scene_tracks(ref(case, cell=2), case)
    off = scene_tracks(ref(case, cell=2, radius=0.0), case)
    print(f"{n} points in two views or more; tracks {on['total']} ({on['total'] / n:.1%}), dropped {on['info'][3]} ({on['info'][3] / n:.1%}); "
          f"radius 0: tracks {off['total']} ({off['total'] / n:.1%}), dropped {off['info'][3]}")
    assert n == 292 and on["total"] >= 0.9 * n and on["info"][3] <= 0.05 * n and off["total"] < 0.75 * n


def test_abi_symbols_sources_and_workspace(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [23, 6]
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "set_keypoints.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "set_keypoints" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()
    ws = built_lib.roma_op_keypoints_from_matches_workspace  # (B, V, P, N, G_total, K)
    assert ws(0, 3, 3, 100, 5000, 100) == 0 and ws(2, 0, 3, 100, 5000, 100) == 0 and ws(2, 3, 3, 100, 0, 100) == 0
    assert ws(2, 3, 3, 100, 5000, 0) == 0 and ws(2, 3, 3, 100, 5000, 65537) == 0 and ws(2, 9, 3, 100, 5000, 100) == 0
    assert ws(1, 2, 1, 10, 3 * (1 << 22), 100) == 0 and ws(70000, 2, 1, 10, 1 << 13, 100) == 0  # beyond the limits: refused
    base = ws(1, 3, 3, 100, 5000, 100)
    assert 0 < base < ws(2, 3, 3, 100, 5000, 100) and base < ws(1, 4, 3, 100, 5000, 100) and base < ws(1, 3, 3, 100, 50000, 100)
    assert base < ws(1, 3, 3, 100, 5000, 1000) and base <= ws(1, 3, 4, 100, 5000, 100)
    assert ws(1, 8, 28, 5000, 8 * 432 * 576, 16384) >= 12 * 8 * 432 * 576 + 16 * 28 * 16384  # 12 bytes a cell, 16 per (pair, keypoint)


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    pairs = (C.c_int * 6)(0, 1, 1, 2, 0, 2)
    sizes = (C.c_int * 6)(480, 640, 480, 640, 480, 640)
    need = lib.roma_op_keypoints_from_matches_workspace(2, 3, 3, 50, 3 * 240 * 320, 100)
    assert need > 0

    def kp(m=p, c=p, pv=pairs, sz=sizes, B=2, V=3, P=3, N=50, cell=2, radius=2.0, K=100, o2o=1, kpts=p, inds=p, kept=p, info=p, ws=p, nws=need):
        return lib.roma_op_keypoints_from_matches(m, c, None, pv, sz, B, V, P, N, cell, radius, K, o2o, kpts, p, p, p, inds, kept, info, ws, nws, None)

    def szs(*v):
        return (C.c_int * 6)(*v)

    cases = [(lambda: kp(kpts=None), "null pointer"), (lambda: kp(m=None), "null pointer"), (lambda: kp(c=None), "null pointer"),
             (lambda: kp(sz=None), "null pointer"), (lambda: kp(pv=None), "null pointer"), (lambda: kp(inds=None), "null pointer"),
             (lambda: kp(V=1), "views"), (lambda: kp(V=9), "views"), (lambda: kp(B=65536), "B must"), (lambda: kp(B=-1), "B must"),
             (lambda: kp(P=65), "pairs"), (lambda: kp(N=-1), "N >= 0"), (lambda: kp(P=64, N=1 << 25), "2^32"),
             (lambda: kp(B=60000, N=50000), "2^30"), (lambda: kp(K=0), "max_kpts"), (lambda: kp(K=65537), "max_kpts"),
             (lambda: kp(cell=0), "cell must"), (lambda: kp(cell=65), "cell must"), (lambda: kp(radius=-0.5), "radius"),
             (lambda: kp(radius=2.5), "radius"), (lambda: kp(radius=float("nan")), "radius"), (lambda: kp(o2o=2), "one_to_one"),
             (lambda: kp(m=8), "16-byte"), (lambda: kp(inds=12), "8-byte"), (lambda: kp(kpts=12), "8-byte"),
             (lambda: kp(sz=szs(480, 640, 0, 640, 480, 640)), "image sizes"), (lambda: kp(sz=szs(480, 640, 480, 65536, 480, 640)), "image sizes"),
             (lambda: kp(sz=szs(480, 640, 4000, 4000, 480, 640), cell=1, radius=1.0), "2^22 cells"),
             (lambda: kp(B=600, sz=szs(2000, 2000, 2000, 2000, 2000, 2000), cell=1, radius=0.0, N=1), "2^28"),
             (lambda: kp(pv=(C.c_int * 6)(0, 1, 1, 3, 0, 2)), "out of range"), (lambda: kp(pv=(C.c_int * 6)(0, 1, -1, 2, 0, 2)), "out of range"),
             (lambda: kp(pv=(C.c_int * 6)(0, 1, 2, 2, 0, 2)), "itself"), (lambda: kp(pv=(C.c_int * 6)(0, 1, 2, 2, 0, 2), N=0), "itself"),
             (lambda: kp(nws=need - 1), "workspace too small"), (lambda: kp(ws=None), "workspace too small")]
    for k, (call, word) in enumerate(cases):
        assert call() != 0 and word in lib.roma_last_error().decode(), (k, word, lib.roma_last_error())
    assert kp(B=0) == 0 and kp(B=0, ws=None, nws=0) == 0  # nothing to do: no launch, no error


def test_python_surface(built_lib):
    import roma_amd
    from roma_amd._lib import RomaHipError
    from roma_amd.matcher import RegressionMatcher
    m, c = torch.zeros((3, 4, 4)), torch.zeros((3, 4))
    pairs, sizes = [(0, 1), (1, 2), (0, 2)], [(48, 64)] * 3
    f = roma_amd.keypoints_from_matches
    with pytest.raises(RomaHipError, match="no CPU fallback"):
        f(m, c, pairs, 3, sizes)
    bad = [lambda: f(m, c, pairs, 9, sizes), lambda: f(m, c, pairs, 1, sizes), lambda: f(m, c, pairs[:2], 3, sizes),
           lambda: f(m, c, [(0, 1), (1, 3), (0, 2)], 3, sizes), lambda: f(m, c, [(0, 1), (1, 1), (0, 2)], 3, sizes),
           lambda: f(m[..., :3], c, pairs, 3, sizes), lambda: f(m.int(), c, pairs, 3, sizes), lambda: f(m, c[:2], pairs, 3, sizes),
           lambda: f(m, c, pairs, 3, sizes[:2]), lambda: f(m, c, pairs, 3, [(0, 64)] * 3), lambda: f(m, c, pairs, 3, [(48, 65536)] * 3),
           lambda: f(m, c, pairs, 3, sizes, cell=0), lambda: f(m, c, pairs, 3, sizes, cell=65), lambda: f(m, c, pairs, 3, sizes, radius=-1.0),
           lambda: f(m, c, pairs, 3, sizes, cell=2, radius=2.5), lambda: f(m, c, pairs, 3, sizes, radius=float("nan")),
           lambda: f(m, c, pairs, 3, sizes, max_kpts=0), lambda: f(m, c, pairs, 3, sizes, max_kpts=65537),
           lambda: f(m, c, pairs, 3, [(4000, 4000)] * 3, cell=1),
           lambda: f(torch.zeros((1, 65, 4, 4)), torch.zeros((1, 65, 4)), [(0, 1)] * 65, 3, sizes)]
    for k, call in enumerate(bad):
        try:
            call()
        except ValueError:
            continue
        pytest.fail(f"bad call {k} raised no ValueError")
    for name in ("keypoints_from_matches", "SetKeypoints"):
        assert name in roma_amd.__all__ and hasattr(roma_amd, name)
    assert roma_amd.SetKeypoints._fields == ("kpts", "score", "num_kpts", "total", "inds", "kept", "info")
    assert callable(RegressionMatcher.set_keypoints) and callable(RegressionMatcher.reconstruct_image_set)
    assert "set_keypoints" in roma_amd.tracks.__doc__ and "match_keypoints" in roma_amd.tracks.__doc__  # both recipes


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_set_keypoints_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "set_keypoints.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/set_keypoints.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == KERNELS, names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 64, k
        assert k["lds"] <= 4 * 4096 + 4 * 256 + 64, k  # the scan: one int per block of a view, the histogram, one int per wave
