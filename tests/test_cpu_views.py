"""The numpy oracles of the multi-view stage - tools/tracks_ref.py against a breadth-first restatement, tools/triangulate_views_ref.py
against exact synthetic geometry - the chain of restatements `reconstruct_views` is held against, and the C ABI of
roma_op_build_tracks / roma_op_triangulate_views without a GPU (argument validation only)."""
import ctypes as C
import glob
import os
import re
from collections import deque

import numpy as np
import pytest
import torch

from conftest import ROOT
from views_cases import (HAND_MADE_INFO, HAND_MADE_TRACKS, SHAPES, chain_errors, hand_made, planted, ref_chain, scene, track_ref, tri_case, tvr,
                         zigzag)

NEW_SYMBOLS = ["roma_op_build_tracks", "roma_op_build_tracks_workspace", "roma_op_triangulate_views"]


def bfs_tracks(c, max_tracks=None, min_views=2):
    """the definition again, by breadth-first search over an adjacency list"""
    V, K = c["V"], c["K"]
    nk = np.full(V, K) if c["num_kpts"] is None else np.clip(c["num_kpts"], 0, K)
    adj = {}
    used = ignored = 0
    for (a, b), rows, mc in zip(c["pairs"], c["inds"], c["match_counts"]):
        for i, j in rows[:mc]:
            if 0 <= i < nk[a] and 0 <= j < nk[b]:
                used += 1
                adj.setdefault((a, int(i)), set()).add((b, int(j)))
                adj.setdefault((b, int(j)), set()).add((a, int(i)))
            else:
                ignored += 1
    seen, comps = set(), []
    for node in sorted(adj, key=lambda n: n[0] * K + n[1]):
        if node in seen:
            continue
        comp, q = [], deque([node])
        seen.add(node)
        while q:
            u = q.popleft()
            comp.append(u)
            for w in adj[u] - seen:
                seen.add(w)
                q.append(w)
        comps.append(comp)  # in ascending order of the smallest id: the first node of a component is its smallest
    good = [cp for cp in comps if len({v for v, _ in cp}) == len(cp)]
    tracks = [cp for cp in good if len(cp) >= min_views]
    T = K if max_tracks is None else max_tracks
    out = np.full((V, T), -1, dtype=np.int32)
    for k, cp in enumerate(tracks[:T]):
        for v, i in cp:
            out[v, k] = i
    return out, len(tracks), (used, ignored, len(comps), len(comps) - len(good))


def _same(c, **kw):
    o = track_ref(c, **kw)
    tracks, total, info = bfs_tracks(c, **kw)
    assert np.array_equal(o["tracks"], tracks) and o["total"] == total and o["info"] == info and o["count"] == min(total, tracks.shape[1])
    present = o["tracks"] >= 0
    assert np.isnan(o["kpts"][~present]).all()
    for v in range(c["V"]):
        assert np.array_equal(o["kpts"][v][present[v]], c["x"][v][o["tracks"][v][present[v]]])
    return o


def test_tracks_ref_on_the_hand_made_case():
    o = _same(hand_made())
    assert o["total"] == 2 and np.array_equal(o["tracks"][:, :2], HAND_MADE_TRACKS) and o["info"] == HAND_MADE_INFO
    assert (o["tracks"][:, 2:] == -1).all()


@pytest.mark.parametrize("permute", [False, True])
def test_tracks_ref_on_the_zigzag(permute):
    o = _same(zigzag(permute))
    assert o["total"] == 10 and o["info"] == (2059, 0, 11, 1)
    assert np.array_equal(o["tracks"][0, :10], 1025 + np.arange(10)) and np.array_equal(o["tracks"][1, :10], 1034 - np.arange(10))


@pytest.mark.parametrize("V,K,seed", [(8, 257, 0), (3, 40, 1), (5, 64, 2), (2, 30, 3)])
def test_tracks_ref_on_random_graphs_and_invariance(V, K, seed):
    c = planted(V, K, seed, num_kpts=None if seed % 2 == 0 else [K - v for v in range(V)], all_pairs=seed != 2)
    o = _same(c)
    assert o["total"] > 0 and (o["info"][3] > 0 or K < 257)  # the large graph has components that hold a view twice
    _same(c, max_tracks=max(1, o["total"] // 2))
    _same(c, min_views=min(3, V))
    # the result depends on the set of edges alone: shuffle the rows and the pairs, duplicate rows
    g = np.random.default_rng(seed + 10)
    P, M = c["inds"].shape[:2]
    d = dict(c)
    order = g.permutation(P)
    inds = np.full((P, 2 * M, 2), -1, dtype=np.int32)
    counts = np.zeros(P, dtype=np.int32)
    for q, p in enumerate(order):
        rows = c["inds"][p, :c["match_counts"][p]]
        rows = np.concatenate([rows, rows[g.random(len(rows)) < 0.3]])
        rows = rows[g.permutation(len(rows))]
        inds[q, :len(rows)], counts[q] = rows, len(rows)
    d.update(pairs=c["pairs"][order], inds=inds, match_counts=counts)
    o2 = track_ref(d)
    assert np.array_equal(o2["tracks"], o["tracks"]) and o2["total"] == o["total"] and o2["info"][2:] == o["info"][2:]
    assert np.array_equal(o2["kpts"], o["kpts"], equal_nan=True)


@pytest.mark.parametrize("name", list(SHAPES))
def test_triangulate_views_ref_recovers_exact_geometry(name):
    """every point seen in two views or more is valid, nothing is trimmed, and the point is the scene's within the f32 rounding
    of the pixels: 1.7e-5 measured at the worst (v3), asserted at 1e-4"""
    for trim in (False, True):
        s, o, left_out = tri_case(name, False, trim)
        seen = np.isfinite(s["kpts"]).all(axis=2)
        two = seen.sum(axis=0) >= 2
        err = np.abs(o["points"] - s["X"])[two].max()
        print(f"{name}: {two.sum()} of {len(two)} points, error {err:.2e}, stats {o['stats']}")
        assert (o["flags"][two] == 0).all() and (o["flags"][~two] == tvr.DEGENERATE).all() and np.isnan(o["points"][~two]).all()
        assert o["stats"][6] == 0 and np.array_equal(o["used"], seen & two[None]) and err < 1e-4
        assert o["stats"][:3] == (len(two), int(two.sum()), int((~two).sum())) and not left_out.any()
        assert np.isfinite(o["reproj"][seen & two[None]]).all() and np.isnan(o["reproj"][~(seen & two[None])]).all()
        assert (o["parallax"][two] > 0).all() and np.isnan(o["parallax"][~two]).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_triangulate_views_ref_on_noisy_scenes(name):
    """0.5 px of noise, 10 % outliers, max_reproj = 2: the cost never rises above the midpoint's, no point that keeps two true
    observations in use has a flag set, trimming does not lose valid tracks, and no trimming decision of the oracle is within
    1e-4 of the threshold"""
    s, off, _ = tri_case(name, True, False)
    s, on, left_out = tri_case(name, True, True)
    for o in (off, on):
        fit = (o["flags"] & 3) == 0
        assert (o["cost"][fit] <= o["cost0"][fit]).all() and fit.sum() > 0
    kept = (on["used"] & s["truth"]).sum(axis=0) >= 2
    print(f"{name}: valid {on['stats'][1]} with trimming, {off['stats'][1]} without; {on['stats'][6]} observations trimmed; "
          f"{kept.sum()} points keep two true observations or more in use")
    assert kept.sum() > 0 and (on["flags"][kept] == 0).all()
    assert on["stats"][1] >= off["stats"][1] and not left_out.any()
    if name != "v2":
        assert on["stats"][6] > 0 and on["stats"][1] > off["stats"][1]


def test_triangulate_views_ref_edge_cases():
    s = scene(3, 12, 4)
    kp = s["kpts"].astype(np.float32)
    kp[1, 0] = kp[0, 0]  # two identical rays from two views with the same pose
    R, t, K = s["R"].copy(), s["t"].copy(), s["K"].copy()
    R[1], t[1], K[1] = R[0], t[0], K[0]
    kp[2, 0], kp[1, 1:] = np.nan, np.nan  # the other points are seen from views 0 and 2
    o = tvr.triangulate(kp, K, R, t)
    assert o["flags"][0] == tvr.DEGENERATE and np.isnan(o["points"][0]).all() and not o["used"][:, 0].any()
    assert (o["flags"][1:] == 0).all() and np.isfinite(o["points"][1:]).all()
    # a view that is not valid is a view whose observations are NaN
    a = tvr.triangulate(s["kpts"].astype(np.float32), s["K"], s["R"], s["t"], view_valid=[1, 0, 1])
    k2 = s["kpts"].astype(np.float32)
    k2[1] = np.nan
    b = tvr.triangulate(k2, s["K"], s["R"], s["t"])
    for key in ("points", "reproj", "used", "parallax", "flags"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    # counts and valid: skipped rows
    c = tvr.triangulate(k2, s["K"], s["R"], s["t"], count=5)
    assert (c["flags"][5:] == tvr.SKIPPED).all() and np.isnan(c["points"][5:]).all() and c["stats"][0] == 5
    assert tvr.triangulate(k2, s["K"], s["R"], s["t"], valid=False)["stats"] == (0,) * 8
    # a point behind a camera, and one too close to parallel for min_parallax
    far = tvr.triangulate(s["kpts"].astype(np.float32), s["K"], s["R"], s["t"], max_depth=4.0, min_parallax=60.0)
    assert (far["flags"] & tvr.PARALLAX).all() and (far["flags"] & tvr.CHEIRALITY).any() and np.isfinite(far["points"]).all()


def test_reference_chain_of_reconstruct_views():
    """the numpy chain on scene(4, 300, seed 5, missing 0.2): its pose errors are what the device is held to (twice them, with
    the exact-data figure as the floor)"""
    for noisy in (False, True):
        r = ref_chain(5, noisy)
        er, et = chain_errors(5, noisy)
        print(f"{'noisy' if noisy else 'exact'}: rotation {er:.3e} deg, translation direction {et:.3e} deg, cost {r['cost'][0]:.3e} -> {r['cost'][1]:.3e}")
        assert r["view_ok"].all() and r["cost"][1] <= r["cost"][0] and er < (0.5 if noisy else 1e-3) and et < (2.0 if noisy else 1e-2)
    r = ref_chain(5, True, 3)
    assert r["view_ok"].tolist() == [True, True, True, False] and np.array_equal(r["R"][3], np.eye(3))


def test_abi_symbols_and_sources(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [20, 5, 23]
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    for src in ("tracks", "triangulate_views"):
        assert f"{src}.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
        assert src not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()
    ws = built_lib.roma_op_build_tracks_workspace
    assert ws(0, 3, 100, 3, 50) == 0 and ws(2, 0, 100, 3, 50) == 0 and ws(2, 3, 0, 3, 50) == 0 and ws(2, 3, 65537, 3, 50) == 0
    assert 0 < ws(1, 3, 100, 3, 50) < ws(1, 3, 1000, 3, 50) < ws(4, 3, 1000, 3, 50)
    assert ws(1, 8, 16384, 28, 4096) >= 8 * 16384 * 4  # a label for every keypoint


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    pairs = (C.c_int * 6)(0, 1, 1, 2, 0, 2)
    need = lib.roma_op_build_tracks_workspace(2, 3, 100, 3, 50)

    def bt(inds=p, pv=pairs, B=2, V=3, K=100, P=3, M=50, T=100, mv=2, x=p, out_x=p, ws=p, nws=need, tracks=p):
        return lib.roma_op_build_tracks(inds, pv, None, None, x, B, V, K, P, M, T, mv, tracks, out_x, p, p, p, ws, nws, None)

    def tv(kpts=p, B=2, V=3, N=100, reproj=2.0, par=0.0, depth=10.0, mv=2, gn=3, trim=1):
        return lib.roma_op_triangulate_views(kpts, None, p, p, None, None, None, B, V, N, reproj, par, depth, mv, gn, trim, p, p, p, p, p, p, None)

    cases = [(lambda: bt(tracks=None), "null pointer"), (lambda: bt(inds=None), "null pointer"), (lambda: bt(V=0), "views"),
             (lambda: bt(V=1), "views"), (lambda: bt(V=9), "views"), (lambda: bt(B=65536), "B must"), (lambda: bt(K=65537), "keypoints"),
             (lambda: bt(P=65), "pairs"), (lambda: bt(M=-1), "negative"), (lambda: bt(T=-1), "negative"), (lambda: bt(mv=1), "min_views"),
             (lambda: bt(mv=4), "min_views"), (lambda: bt(x=None), "go together"), (lambda: bt(inds=12), "aligned"),
             (lambda: bt(pv=(C.c_int * 6)(0, 1, 1, 3, 0, 2)), "out of range"), (lambda: bt(pv=(C.c_int * 6)(0, 1, -1, 2, 0, 2)), "out of range"),
             (lambda: bt(pv=(C.c_int * 6)(0, 1, 2, 2, 0, 2)), "itself"), (lambda: bt(pv=(C.c_int * 6)(0, 1, 1, 3, 0, 2), M=0), "out of range"),
             (lambda: bt(pv=(C.c_int * 6)(0, 1, 1, 1, 0, 2), M=0, inds=None), "itself"), (lambda: bt(pv=None, M=0), "null pointer"),
             (lambda: bt(nws=need - 1), "workspace too small"),
             (lambda: bt(ws=None), "workspace too small"), (lambda: bt(B=60000, M=50000), "2^30"),
             (lambda: tv(kpts=None), "null pointer"), (lambda: tv(V=0), "views"), (lambda: tv(V=9), "views"), (lambda: tv(B=65536), "B must"),
             (lambda: tv(N=-1), "N >= 0"), (lambda: tv(B=60000, V=8, N=5000), "2^31"), (lambda: tv(reproj=-1.0), "threshold"),
             (lambda: tv(par=-0.5), "threshold"), (lambda: tv(depth=float("nan")), "threshold"), (lambda: tv(mv=1), "min_views"),
             (lambda: tv(mv=4), "min_views"), (lambda: tv(gn=11), "gn_steps"), (lambda: tv(gn=-1), "gn_steps"), (lambda: tv(trim=2), "trim"),
             (lambda: tv(kpts=12), "aligned")]
    for k, (call, word) in enumerate(cases):
        assert call() != 0 and word in lib.roma_last_error().decode(), (k, word, lib.roma_last_error())
    # nothing to do: no launch, no error
    assert bt(B=0) == 0 and tv(B=0) == 0 and tv(N=0) == 0


def test_python_argument_errors(built_lib):
    import roma_amd
    from roma_amd._lib import RomaHipError
    inds = torch.zeros((3, 4, 2), dtype=torch.int32)
    pairs = [(0, 1), (1, 2), (0, 2)]
    x, K = torch.zeros((3, 8, 2)), np.eye(3)
    R, t = torch.eye(3).expand(3, 3, 3), torch.zeros(3, 3)
    host = [lambda: roma_amd.build_tracks(inds, pairs, 3, kpts=x), lambda: roma_amd.build_tracks(inds, pairs, 3, kpts_per_view=8),
            lambda: roma_amd.triangulate_views(x, K, R, t), lambda: roma_amd.reconstruct_views(x, K, 1e-3, 2.0)]
    for call in host:
        with pytest.raises(RomaHipError, match="no CPU fallback"):
            call()
    bad = [lambda: roma_amd.build_tracks(inds, pairs, 9, kpts=x), lambda: roma_amd.build_tracks(inds, pairs, 1, kpts=x),
           lambda: roma_amd.build_tracks(inds, pairs[:2], 3, kpts=x), lambda: roma_amd.build_tracks(inds, [(0, 1), (1, 3), (0, 2)], 3, kpts=x),
           lambda: roma_amd.build_tracks(inds, [(0, 1), (1, 1), (0, 2)], 3, kpts=x), lambda: roma_amd.build_tracks(inds[..., :1], pairs, 3, kpts=x),
           lambda: roma_amd.build_tracks(inds.float(), pairs, 3, kpts=x), lambda: roma_amd.build_tracks(inds, pairs, 3, kpts=x[:2]),
           lambda: roma_amd.build_tracks(inds, pairs, 3), lambda: roma_amd.build_tracks(inds, pairs, 3, kpts_per_view=65537),
           lambda: roma_amd.build_tracks(inds, pairs, 3, kpts=torch.zeros((3, 65537, 2))),
           lambda: roma_amd.build_tracks(inds, pairs, 3, kpts=x, min_views=1), lambda: roma_amd.build_tracks(inds, pairs, 3, kpts=x, max_tracks=-1),
           lambda: roma_amd.build_tracks(torch.zeros((1, 65, 4, 2), dtype=torch.int32), [(0, 1)] * 65, 3, kpts_per_view=8),
           lambda: roma_amd.triangulate_views(x[..., :1], K, R, t), lambda: roma_amd.triangulate_views(x[:1], K, R, t),
           lambda: roma_amd.triangulate_views(torch.zeros((9, 8, 2)), K, R, t), lambda: roma_amd.triangulate_views(x, K, R, t, gn_steps=11),
           lambda: roma_amd.triangulate_views(x, K, R, t, min_views=1), lambda: roma_amd.triangulate_views(x, K, R, t, max_reproj=-1.0),
           lambda: roma_amd.triangulate_views(x, K, R, t, min_parallax=float("nan")),
           lambda: roma_amd.reconstruct_views(x[:1], K, 1e-3, 2.0), lambda: roma_amd.reconstruct_views(x[0], K, 1e-3, 2.0)]
    for k, call in enumerate(bad):
        try:
            call()
        except ValueError:
            continue
        pytest.fail(f"bad call {k} raised no ValueError")
    for name in ("build_tracks", "Tracks", "triangulate_views", "ViewsTriangulation", "reconstruct_views", "ViewsReconstruction"):
        assert name in roma_amd.__all__ and hasattr(roma_amd, name)


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_views_kernels_have_no_spills_and_no_scratch(build):
    for src, kernel, lds in (("tracks", "build_tracks_kernel", 1024), ("triangulate_views", "triangulate_views_kernel", 2048)):
        obj = os.path.join(ROOT, "roma_amd", "csrc", build, f"{src}.o")
        if not glob.glob(obj):
            pytest.skip(f"{build}/{src}.o not built")
        import kernel_resources
        ks = kernel_resources.kernels(obj)
        names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
        assert names == [kernel], names
        for k in ks:
            assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] <= lds, k
            assert k["vgpr"] <= 128, k  # build_tracks runs 1024 threads a workgroup: four waves a SIMD
