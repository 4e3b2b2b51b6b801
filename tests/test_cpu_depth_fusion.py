"""The numpy oracle of dense depth fusion - tools/depth_fusion_ref.py against a hand-made case whose outputs are written out, against
a scalar restatement of the definition, and for its properties on a closed-form scene - the margins of every case the GPU file
compares bit for bit, and the C ABI of roma_op_fuse_depth_maps / roma_op_relative_poses without a GPU (argument validation only)."""
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from depth_fusion_cases import (HAND_KW, RANDOM_PAIRS, WIDE_CUT, chain_case, chain_ref_default, check_hand_made, dfr, gpu_margins, hand_made,
                                operator_case, plane_distance, random_case, ref, wide_case, wide_ref)

NEW_SYMBOLS = ["roma_op_fuse_depth_maps", "roma_op_fuse_depth_maps_workspace", "roma_op_relative_poses"]
f32 = np.float32


def scalar_fuse(c, rel_thresh=0.01, min_support=2, min_consistent=1, max_violations=0, dedupe=True):
    """the definition again, pixel by pixel in Python floats: depth, weight, support, seen, violated, state, source"""
    z_all, flags, cert = c["points"][..., 2], c["flags"], c["certainty"]
    K, R, t, pairs = c["cameras"], c["R"], c["t"], c["pairs"]
    V, (P, H, Wd) = len(K), z_all.shape
    W = Wd // 2 if c["symmetric"] else Wd
    rel = float(rel_thresh)
    depth = np.full((V, H, W), np.nan, dtype=f32)
    weight, support = np.zeros((V, H, W), dtype=f32), np.zeros((V, H, W), dtype=np.uint8)
    for v in range(V):
        slots = [(p, h) for p, pr in enumerate(pairs) for h in range(2 if c["symmetric"] else 1) if pr[h] == v]
        for r in range(H):
            for col in range(W):
                hyp = []
                for p, h in slots:
                    z, f = float(z_all[p, r, h * W + col]), int(flags[p, r, h * W + col])
                    w = 1.0 if cert is None else float(cert[p, r, h * W + col])
                    if f == 0 and math.isfinite(z) and z > 0 and math.isfinite(w) and w > 0:
                        hyp.append((z, w))
                best = (0, 0.0, 0.0)
                for zk, _ in hyp:
                    n, s, m = 0, 0.0, 0.0
                    for zl, wl in hyp:
                        if abs(zl - zk) <= rel * min(zl, zk):
                            n, s, m = n + 1, s + wl, m + wl * zl
                    if n > best[0] or (n == best[0] and s > best[1]):
                        best = (n, s, m)
                support[v, r, col] = best[0]
                if best[0] >= min_support:
                    depth[v, r, col], weight[v, r, col] = f32(best[2] / best[1]), f32(best[1])

    def world(v, r, col):
        fx, fy, cx, cy = K[v][0, 0], K[v][1, 1], K[v][0, 2], K[v][1, 2]
        z = float(depth[v, r, col])
        d = [z * (((col + 0.5) - cx) / fx) - t[v][0], z * (((r + 0.5) - cy) / fy) - t[v][1], z - t[v][2]]
        return [(R[v][0, i] * d[0] + R[v][1, i] * d[1]) + R[v][2, i] * d[2] for i in range(3)]

    def project(u, X):
        y = [((R[u][i, 0] * X[0] + R[u][i, 1] * X[1]) + R[u][i, 2] * X[2]) + t[u][i] for i in range(3)]
        if y[2] == 0.0 or not math.isfinite(y[2]):
            return y[2], math.nan, math.nan
        return y[2], (K[u][0, 0] * (y[0] / y[2]) + K[u][0, 2]) - 0.5, (K[u][1, 1] * (y[1] / y[2]) + K[u][1, 2]) - 0.5

    seen, violated = np.zeros((V, H, W), dtype=np.uint8), np.zeros((V, H, W), dtype=np.uint8)
    keep = np.zeros((V, H, W), dtype=bool)
    for v in range(V):
        for r in range(H):
            for col in range(W):
                if np.isnan(depth[v, r, col]):
                    continue
                X = world(v, r, col)
                for u in range(V):
                    if u == v:
                        continue
                    pz, gx, gy = project(u, X)
                    if not pz > 0.0 or not (math.isfinite(gx) and math.isfinite(gy)):
                        continue
                    x0, y0 = math.floor(gx), math.floor(gy)
                    if not (0 <= x0 and x0 + 1 <= W - 1 and 0 <= y0 and y0 + 1 <= H - 1):
                        continue
                    n4 = [float(depth[u, y0 + dy, x0 + dx]) for dy in (0, 1) for dx in (0, 1)]
                    if any(math.isnan(x) for x in n4):
                        continue
                    ax, ay = gx - x0, gy - y0
                    d = (n4[0] * (1.0 - ax) + n4[1] * ax) * (1.0 - ay) + (n4[2] * (1.0 - ax) + n4[3] * ax) * ay
                    e = (pz - d) / d
                    if abs(e) <= rel:
                        seen[v, r, col] |= 1 << u
                    if e < -rel:
                        violated[v, r, col] |= 1 << u
                keep[v, r, col] = bin(seen[v, r, col]).count("1") >= min_consistent and bin(violated[v, r, col]).count("1") <= max_violations
    state = keep.astype(np.uint8)
    source = []
    for v in range(V):
        for r in range(H):
            for col in range(W):
                if not keep[v, r, col]:
                    continue
                X = world(v, r, col)
                for u in range(v if dedupe else 0):
                    if not (seen[v, r, col] >> u) & 1:
                        continue
                    _, gx, gy = project(u, X)
                    nx, ny = math.floor(gx + 0.5), math.floor(gy + 0.5)
                    if 0 <= nx <= W - 1 and 0 <= ny <= H - 1 and keep[u, ny, nx]:
                        state[v, r, col] |= 2
                if state[v, r, col] == 1:
                    source.append((v, r * W + col))
    return {"depth": depth, "weight": weight, "support": support, "seen": seen, "violated": violated, "state": state,
            "source": np.asarray(source, dtype=np.int32).reshape(-1, 2)}


def _same_as_scalar(c, **kw):
    o, s = ref(c, **kw), scalar_fuse(c, **kw)
    for k in ("depth", "weight"):
        assert np.array_equal(o[k].view(np.int32), s[k].view(np.int32)), k
    for k in ("support", "seen", "violated", "state"):
        assert np.array_equal(o[k], s[k]), k
    assert o["total"] == len(s["source"]) and np.array_equal(o["source"][:o["count"]], s["source"])
    return o


@pytest.mark.parametrize("dedupe", [True, False])
def test_restatement_on_the_hand_made_case(dedupe):
    """a 2-against-1 vote, an n tie decided by weight, a full tie decided by slot, a pixel below min_support, a violation, an
    occlusion and a duplicate: depth_fusion_cases.HAND_EXPECTED spells every pixel out"""
    kw = dict(HAND_KW, dedupe=dedupe)
    check_hand_made(ref(hand_made(), max_points=4, **kw), dedupe)
    _same_as_scalar(hand_made(), **kw)


@pytest.mark.parametrize("kw", [dict(), dict(rel_thresh=0.05, min_support=1, min_consistent=2), dict(min_support=3, min_consistent=0, dedupe=False),
                                dict(max_violations=1)])
def test_restatement_equals_the_scalar_definition(kw):
    o = _same_as_scalar(operator_case(4, 9, 13, RANDOM_PAIRS, 21), **kw)
    assert o["stats"][1] > 0 and (o["stats"][2] > 0 or kw.get("min_support") == 3)
    o = _same_as_scalar(operator_case(3, 7, 10, [(0, 1), (2, 1)], 22, symmetric=False, with_cert=False), **kw)


def test_exact_hypotheses_fuse_to_the_true_depth():
    """Every slot holds fl32(true depth): a relative error of at most 2^-24.  The weighted mean of values within 2^-24 of z stays
    within 2^-24 (1 + O(2^-52)) of it in float64, and its rounding to float32 adds 2^-24 of the result: |depth - z| <= 2^-23 z,
    with 2^-40 z for the float64 terms and the second-order product.  Every pixel with min_support usable slots or more is fused."""
    c = operator_case(4, 24, 40, RANDOM_PAIRS, 31, noise=0.0, outliers=0.0)
    o = ref(c, min_support=2)
    usable = np.zeros((4, 24, 40), dtype=np.int64)
    for v, slots in enumerate(dfr.slots_of(c["pairs"], 4, True)):
        for p, h in slots:
            sl = np.s_[p, :, h * 40:(h + 1) * 40]
            usable[v] += (c["flags"][sl] == 0) & (c["certainty"][sl] > 0)
    fused = ~np.isnan(o["depth"])
    assert np.array_equal(fused, usable >= 2) and np.array_equal(o["support"], usable) and fused.sum() > 3000 and (~fused).sum() > 0
    err = np.abs(o["depth"].astype(np.float64) - c["truth"])[fused] / c["truth"][fused]
    print(f"largest relative error {err.max():.3e} (bound {2.0 ** -23 + 2.0 ** -40:.3e})")
    assert err.max() <= 2.0 ** -23 + 2.0 ** -40


def test_one_planted_outlier_per_pixel_changes_no_depth():
    """V = 4 with all six pairs: three slots a pixel, all usable, exact.  One slot of every pixel becomes an outlier (x 0.4 .. 0.8 or
    x 1.25 .. 2): the two others still agree, and the mean of equal float32 values is that value - the depth keeps its bits."""
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    c = operator_case(4, 12, 20, pairs, 32, noise=0.0, outliers=0.0, flagged=0.0)
    c["certainty"] = np.maximum(c["certainty"], f32(0.2))
    clean = ref(c)
    assert (clean["support"] == 3).all()
    g = np.random.default_rng(32)
    d = dict(c, points=c["points"].copy())
    slots = dfr.slots_of(pairs, 4, True)
    for v in range(4):
        pick = g.integers(0, 3, (12, 20))
        factor = np.where(g.random((12, 20)) < 0.5, g.uniform(0.4, 0.8, (12, 20)), g.uniform(1.25, 2.0, (12, 20)))
        for k, (p, h) in enumerate(slots[v]):
            sl = np.s_[p, :, h * 20:(h + 1) * 20, 2]
            d["points"][sl] = np.where(pick == k, d["points"][sl] * factor, d["points"][sl]).astype(f32)
    planted = ref(d)
    assert (planted["support"] == 2).all() and np.array_equal(planted["depth"].view(np.int32), clean["depth"].view(np.int32))


def test_an_unusable_slot_changes_nothing():
    c = random_case()
    o = ref(c)
    for extra, fill in (("flag", None), ("nan", np.nan), ("negative", -3.0), ("no certainty", None)):
        d = dict(c, pairs=c["pairs"] + [(2, 3)])
        d["points"] = np.concatenate([c["points"], np.full_like(c["points"][:1], 5.0 if fill is None else fill)])
        d["flags"] = np.concatenate([c["flags"], np.full_like(c["flags"][:1], 8 if extra == "flag" else 0)])
        d["certainty"] = np.concatenate([c["certainty"], np.full_like(c["certainty"][:1], 0.0 if extra == "no certainty" else 1.0)])
        e = ref(d)
        for k in ("depth", "weight", "support", "seen", "violated", "state", "points", "cloud_weight", "source"):
            assert np.array_equal(o[k], e[k], equal_nan=True), (extra, k)
        assert o["stats"] == e["stats"] and o["total"] == e["total"]


def test_relative_poses_restatement():
    c = random_case()
    Rij, tij = dfr.relative_poses(c["R"], c["t"], c["pairs"])
    for p, (i, j) in enumerate(c["pairs"]):
        assert np.allclose(Rij[p], c["R"][j] @ c["R"][i].T, atol=1e-15) and np.allclose(tij[p], c["t"][j] - Rij[p] @ c["t"][i], atol=1e-15)
        X = np.array([0.3, -0.2, 5.0])
        assert np.allclose(Rij[p] @ (c["R"][i] @ X + c["t"][i]) + tij[p], c["R"][j] @ X + c["t"][j], atol=1e-14)


def test_margins_of_every_case_the_gpu_file_compares():
    """no decision of the restatement - support, seen / violated, the floor of a grid position - lies within 1e-9 (relative) of its
    threshold in any case tests/test_gpu_depth_fusion.py compares bit for bit: a mismatch there is a defect, not a borderline case"""
    worst = min(gpu_margins(), key=lambda x: x[1])
    print(f"smallest margin {worst[1]:.3e} ({worst[0]})")
    for name, m in gpu_margins():
        assert m > 1e-9, (name, m)


def test_wide_case_has_more_blocks_than_the_scan_has_threads():
    """the case of the GPU file that gives every thread of the scan kernel two block counts: more than 1024 blocks of 256 pixels, a
    total above the cut, points of the first and of the last view"""
    c, o = wide_case(), wide_ref()
    assert 1024 < c["V"] * -(-c["H"] * c["W"] // 256) <= 2048
    views = o["source"][:o["count"], 0]
    assert o["total"] > WIDE_CUT and (views == 0).any() and (views == 7).any()
    assert wide_ref(WIDE_CUT)["count"] == WIDE_CUT and wide_ref(WIDE_CUT)["total"] == o["total"]


def test_reference_chain_on_the_scene():
    """ground-truth warps of four views of mixed image sizes through the chain of restatements.  Reported, not gated beyond
    sanity: the distance of the emitted points to the true surfaces and the share of the pixels the cloud represents."""
    c, o = chain_case(), chain_ref_default()
    n = o["count"]
    dist = plane_distance(o["points"][:n])
    pixels = c["V"] * c["H"] * c["W"]
    kept, dup = o["stats"][2], o["stats"][3]
    print(f"{pixels} pixels: fused {o['stats'][1]} ({o['stats'][1] / pixels:.1%}), kept {kept} ({kept / pixels:.1%}), duplicates {dup}, emitted {n}; "
          f"distance to the true surfaces: median {np.median(dist):.2e}, largest {dist.max():.2e}")
    assert n == kept - dup and n > 1000 and kept > 0.6 * pixels and dist.max() < 1e-5


def test_abi_symbols_and_sources(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [40, 4, 9]
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "depth_fusion.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "depth_fusion" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()
    ws = built_lib.roma_op_fuse_depth_maps_workspace
    assert ws(0, 3, 24, 40) == 0 and ws(1, 1, 24, 40) == 0 and ws(1, 9, 24, 40) == 0 and ws(1, 3, 0, 40) == 0 and ws(65536, 3, 24, 40) == 0
    assert 0 < ws(1, 3, 24, 40) < ws(1, 3, 240, 400) < ws(4, 3, 240, 400)
    assert ws(1, 8, 864, 864) >= 8 * 864 * 864  # a byte for every pixel


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    pv3 = (C.c_int * 6)(0, 1, 1, 2, 0, 2)
    need = lib.roma_op_fuse_depth_maps_workspace(2, 3, 24, 40)
    off = (C.c_longlong * 6)(*range(6))
    sz = (C.c_int * 12)(*([4] * 12))

    def fd(points=p, pv=pv3, cam=p, images=None, offs=None, sizes=None, B=2, V=3, P=3, H=24, W=40, sym=1, rel=0.01, ms=2, mc=1, mv=0, dd=1,
           K=100, depth=p, colors=None, stats=p, ws=p, nws=need):
        return lib.roma_op_fuse_depth_maps(points, p, None, pv, cam, p, p, None, None, images, offs, sizes, B, V, P, H, W, sym, rel, ms, mc, mv,
                                           dd, K, depth, p, p, p, p, p, p, colors, p, p, p, p, stats, ws, nws, None)

    def rp(R=p, pv=pv3, B=2, V=3, P=3, out=p):
        return lib.roma_op_relative_poses(R, p, pv, B, V, P, out, p, None)

    cases = [(lambda: fd(points=None), "null pointer"), (lambda: fd(pv=None), "null pointer"), (lambda: fd(cam=None), "null pointer"),
             (lambda: fd(depth=None), "null pointer"), (lambda: fd(stats=None), "null pointer"), (lambda: fd(V=1), "views"),
             (lambda: fd(V=9), "views"), (lambda: fd(P=0), "pairs"), (lambda: fd(P=65), "pairs"), (lambda: fd(B=-1), "B must"),
             (lambda: fd(B=65536), "B must"), (lambda: fd(H=0), "positive"), (lambda: fd(W=0), "positive"), (lambda: fd(sym=2), "symmetric"),
             (lambda: fd(dd=2), "dedupe"), (lambda: fd(rel=-0.1), "rel_thresh"), (lambda: fd(rel=float("nan")), "rel_thresh"),
             (lambda: fd(ms=0), "min_support"), (lambda: fd(ms=15), "min_support"), (lambda: fd(mc=-1), "min_consistent"),
             (lambda: fd(mc=8), "min_consistent"), (lambda: fd(mv=-1), "max_violations"), (lambda: fd(K=-1), "max_points"),
             (lambda: fd(pv=(C.c_int * 6)(0, 1, 1, 3, 0, 2)), "out of range"), (lambda: fd(pv=(C.c_int * 6)(0, 1, -1, 2, 0, 2)), "out of range"),
             (lambda: fd(pv=(C.c_int * 6)(0, 1, 2, 2, 0, 2)), "itself"), (lambda: fd(pv=(C.c_int * 6)(0, 1, 1, 2, 0, 1)), "twice"),
             (lambda: fd(images=p), "go together"), (lambda: fd(images=p, offs=off), "go together"), (lambda: fd(colors=p), "colour source"),
             (lambda: fd(B=60000, H=240, W=400), "2^31"), (lambda: fd(K=2 ** 30), "2^31"),
             (lambda: fd(B=50, images=p, offs=off, sizes=sz, colors=p), "128"),
             (lambda: fd(images=p, offs=off, sizes=(C.c_int * 12)(*([4] * 11 + [0])), colors=p), "sizes must be positive"),
             (lambda: fd(images=p, offs=(C.c_longlong * 6)(0, 1, 2, 3, 4, -5), sizes=sz, colors=p), "offsets not negative"),
             (lambda: fd(nws=need - 1), "workspace too small"), (lambda: fd(ws=None), "workspace too small"),
             (lambda: rp(R=None), "null pointer"), (lambda: rp(out=None), "null pointer"), (lambda: rp(V=1), "views"), (lambda: rp(V=9), "views"),
             (lambda: rp(P=0), "pairs"), (lambda: rp(P=65), "pairs"), (lambda: rp(B=65536), "B must"),
             (lambda: rp(pv=(C.c_int * 6)(0, 1, 1, 3, 0, 2)), "out of range"), (lambda: rp(pv=(C.c_int * 6)(0, 1, 1, 1, 0, 2)), "itself")]
    for k, (call, word) in enumerate(cases):
        assert call() != 0 and word in lib.roma_last_error().decode(), (k, word, lib.roma_last_error())
    # (1, 0) after (0, 1) is no repetition; nothing to do: no launch, no error
    assert fd(B=0, pv=(C.c_int * 6)(0, 1, 1, 0, 0, 2)) == 0 and rp(B=0) == 0


def test_python_argument_errors(built_lib):
    import roma_amd
    from roma_amd._lib import RomaHipError
    pairs = [(0, 1), (1, 2), (0, 2)]
    pts, flg, cert = torch.zeros((3, 4, 10, 3)), torch.zeros((3, 4, 10), dtype=torch.uint8), torch.ones((3, 4, 10))
    K, R, t = np.eye(3), torch.eye(3).expand(3, 3, 3), torch.zeros(3, 3)
    fuse, rel = roma_amd.fuse_depth_maps, roma_amd.relative_poses
    for call in (lambda: fuse(pts, flg, cert, pairs, K, R, t), lambda: rel(R, t, pairs)):
        with pytest.raises(RomaHipError, match="no CPU fallback"):
            call()
    bad = [lambda: fuse(pts, flg, cert, pairs, K, R[:1], t[:1]), lambda: fuse(pts, flg, cert, pairs, K, torch.eye(3).expand(9, 3, 3), torch.zeros(9, 3)),
           lambda: fuse(pts, flg, cert, pairs, K, R, t[:2]), lambda: fuse(pts, flg, cert, pairs[:2], K, R, t),
           lambda: fuse(pts, flg, cert, [(0, 1), (1, 3), (0, 2)], K, R, t), lambda: fuse(pts, flg, cert, [(0, 1), (1, 1), (0, 2)], K, R, t),
           lambda: fuse(pts, flg, cert, [(0, 1), (1, 2), (0, 1)], K, R, t), lambda: fuse(pts[..., :2], flg, cert, pairs, K, R, t),
           lambda: fuse(pts, flg[:, :3], cert, pairs, K, R, t), lambda: fuse(pts, flg, cert[:, :3], pairs, K, R, t),
           lambda: fuse(pts[:, :, :9], flg[:, :, :9], cert[:, :, :9], pairs, K, R, t, symmetric=True), lambda: fuse(pts, flg, cert, pairs, None, R, t),
           lambda: fuse(pts, flg, cert, pairs, K, R, t, rel_thresh=-1.0), lambda: fuse(pts, flg, cert, pairs, K, R, t, rel_thresh=float("nan")),
           lambda: fuse(pts, flg, cert, pairs, K, R, t, min_support=0), lambda: fuse(pts, flg, cert, pairs, K, R, t, min_support=15),
           lambda: fuse(pts, flg, cert, pairs, K, R, t, min_consistent=8), lambda: fuse(pts, flg, cert, pairs, K, R, t, max_violations=-1),
           lambda: fuse(pts, flg, cert, pairs, K, R, t, max_points=-1), lambda: fuse(pts[None], flg[None], cert[None], pairs, K, R, t),
           lambda: fuse(pts, flg, cert, [], K, R, t), lambda: rel(R, t, [(0, 3)]), lambda: rel(R[0], t, pairs), lambda: rel(R, t, [])]
    for k, call in enumerate(bad):
        try:
            call()
        except ValueError:
            continue
        pytest.fail(f"bad call {k} raised no ValueError")
    for name in ("fuse_depth_maps", "relative_poses", "DenseFusion"):
        assert name in roma_amd.__all__ and hasattr(roma_amd, name)
    for name in ("fuse_image_set", "dense_reconstruct_image_set"):
        assert callable(getattr(roma_amd.RegressionMatcher, name))


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_depth_fusion_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "depth_fusion.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/depth_fusion.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["fuse_check_kernel", "fuse_dedupe_kernel", "fuse_emit_kernel", "fuse_scan_kernel", "fuse_select_kernel",
                     "relative_poses_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] <= 2048, k
        assert k["vgpr"] <= 128, k  # the select kernel keeps 14 slots of (z, w, w z) in registers: four waves a SIMD still fit
