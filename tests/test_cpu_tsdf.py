"""The numpy oracle of the TSDF operators - tools/tsdf_ref.py - against a hand-made case whose volume and mesh are written out, a
scalar restatement in Python floats, and analytic distance fields (topology, orientation, positions and normals within derived
bounds); the margins of every case that the GPU file compares; and, without a GPU, the C ABI of include/roma_hip_tsdf.h: its
table, its exports, its call sites, its refusals, its kernels' resources."""
import ast
import glob
import itertools
import json
import math
import os
import re
import struct
import sys
from ctypes import c_int as C_int, c_longlong as C_longlong

import numpy as np
import pytest
import torch

from conftest import ROOT
import tsdf_cases as tc
from tsdf_cases import tr

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_goldens import abi_classes  # noqa: E402
from roma_amd import _lib  # noqa: E402

NEW_SYMBOLS = ["roma_op_tsdf_integrate", "roma_op_tsdf_extract_mesh_workspace", "roma_op_tsdf_extract_mesh", "roma_op_points_bounds_workspace",
               "roma_op_points_bounds"]


def test_hand_made_case_through_the_reference():
    c = tc.hand_made()
    tsdf, weight, _ = tc.run_ref(c)
    mesh = tr.extract_mesh(tsdf, weight, None, c["origin"], c["voxel_size"], min_weight=0.5)
    tc.check_hand_made(tsdf, weight, mesh)
    # the same views again: the mean does not move, the weight doubles; with max_weight = 1.5 it stops there
    t2, w2, _ = tc.run_ref(c, state=(tsdf, weight, None))
    assert np.array_equal(t2, tsdf) and np.array_equal(w2, 2 * weight)
    assert tc.run_ref(c, state=(tsdf, weight, None), max_weight=1.5)[1].max() == 1.5


# ------------------------------------------------------------------------------------------------- a scalar restatement, in loops
def _f(x):
    return struct.unpack("f", struct.pack("f", x))[0]  # round a Python float to float32


def _scalar_integrate(c):
    nz, ny, nx = c["dims"]
    V, H, W = c["depth"].shape
    T = [[[1.0] * nx for _ in range(ny)] for _ in range(nz)]
    Wt = [[[0.0] * nx for _ in range(ny)] for _ in range(nz)]
    C = [[[[0.0, 0.0, 0.0] for _ in range(nx)] for _ in range(ny)] for _ in range(nz)]
    o, vs, trunc = [float(x) for x in c["origin"]], float(c["voxel_size"]), float(c["trunc"])
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                X = (o[0] + (i + 0.5) * vs, o[1] + (j + 0.5) * vs, o[2] + (k + 0.5) * vs)
                for v in range(V):
                    R, t, K = c["R"][v].tolist(), c["t"][v].tolist(), c["K"][v].tolist()
                    y = [((R[a][0] * X[0] + R[a][1] * X[1]) + R[a][2] * X[2]) + t[a] for a in range(3)]
                    if not y[2] > c["near"]:
                        continue
                    col, row = math.floor(K[0][0] * (y[0] / y[2]) + K[0][2]), math.floor(K[1][1] * (y[1] / y[2]) + K[1][2])
                    if not (0 <= col < W and 0 <= row < H):
                        continue
                    d = float(c["depth"][v, row, col])
                    w = 1.0 if c["depth_weight"] is None else float(c["depth_weight"][v, row, col])
                    if not (math.isfinite(d) and d > 0 and math.isfinite(w) and w > 0):
                        continue
                    sdf = d - y[2]
                    if sdf < -trunc:
                        continue
                    f = _f(min(1.0, sdf / trunc))
                    old, den = Wt[k][j][i], _f(Wt[k][j][i] + w)
                    T[k][j][i] = _f(_f(_f(old * T[k][j][i]) + _f(w * f)) / den)
                    if c["images"] is not None and sdf <= trunc:
                        im = c["images"][v]
                        px = im[((2 * row + 1) * im.shape[0]) // (2 * H), ((2 * col + 1) * im.shape[1]) // (2 * W)]
                        C[k][j][i] = [_f(_f(_f(old * C[k][j][i][a]) + _f(w * float(px[a]))) / den) for a in range(3)]
                    Wt[k][j][i] = min(den, c["max_weight"])
    return np.array(T, dtype=np.float32), np.array(Wt, dtype=np.float32), np.array(C, dtype=np.float32)


def _scalar_mesh(tsdf, weight, origin, vs, min_weight):
    """marching tetrahedra with a dictionary from edges to vertex numbers, and the winding decided by geometry: a triangle is
    turned round when its normal does not point from the inside corners of its tetrahedron to the outside ones"""
    nz, ny, nx = tsdf.shape
    T, Wt = tsdf.astype(np.float64), weight

    def ok(p):
        return 0 <= p[0] < nx and 0 <= p[1] < ny and 0 <= p[2] < nz and Wt[p[2], p[1], p[0]] >= min_weight

    def val(p):
        return T[p[2], p[1], p[0]]
    number, verts = {}, []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for c in range(1, 8):
                    p, q = (i, j, k), (i + (c & 1), j + (c >> 1 & 1), k + (c >> 2))
                    if ok(p) and ok(q) and (val(p) < 0) != (val(q) < 0):
                        s = val(p) / (val(p) - val(q))
                        number[(p, q)] = len(verts)
                        verts.append([origin[a] + ((p[a] + 0.5) + s * (q[a] - p[a])) * vs for a in range(3)])
    faces = []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                for perm in itertools.permutations(range(3)):
                    corner = [[i, j, k]]
                    for a in perm:
                        nxt = list(corner[-1])
                        nxt[a] += 1
                        corner.append(nxt)
                    corner = [tuple(p) for p in corner]
                    if not all(ok(p) for p in corner):
                        continue
                    ins = [n for n in range(4) if val(corner[n]) < 0]
                    out = [n for n in range(4) if n not in ins]
                    if not ins or not out:
                        continue

                    def vert(a, b):
                        return number[(corner[min(a, b)], corner[max(a, b)])]
                    away = np.mean([corner[n] for n in out], axis=0) - np.mean([corner[n] for n in ins], axis=0)
                    if len(ins) == 2:
                        (a, b), (c_, d) = ins, out
                        if sum(x > y for n, x in enumerate((a, b, c_, d)) for y in (a, b, c_, d)[n + 1:]) % 2:  # the cut runs ik - jl, (i, j, k, l) even
                            c_, d = d, c_
                        quad = [vert(a, c_), vert(a, d), vert(b, d), vert(b, c_)]
                        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
                    else:
                        lone, rest = (ins[0], out) if len(ins) == 1 else (out[0], ins)
                        tris = [[vert(lone, n) for n in rest]]
                    for tri in tris:
                        P = np.array([verts[n] for n in tri])
                        if np.cross(P[1] - P[0], P[2] - P[0]) @ away < 0:
                            tri = [tri[0], tri[2], tri[1]]
                        faces.append(tri)
    return np.array(verts), faces


def test_scalar_loops_agree_with_the_reference():
    c = tc.scene_case(2, 9, 11, (6, 5, 4), seed=31)
    ref = tc.run_ref(c)
    mine = _scalar_integrate(c)
    for a, b in zip(ref, mine):
        assert np.array_equal(a, b, equal_nan=True)
    assert 0 < (ref[1] > 0).sum() < ref[1].size and (ref[0] < 0).any()
    # the mesh of that volume and of a small sphere: the same vertices in the same order; the same faces as sets of cyclic triples
    sphere = tc.field("sphere", 8)
    for tsdf, weight, origin, vs, mw in ((ref[0], ref[1], c["origin"], c["voxel_size"], 0.1), (sphere[0], sphere[1], tc.FIELD_ORIGIN, 1.0, 0.5)):
        o = tr.extract_mesh(tsdf, weight, None, origin, vs, min_weight=mw)
        verts, faces = _scalar_mesh(tsdf, weight, origin, vs, mw)
        nv, nf = o["counts"]
        assert nv == len(verts) > 0 and nf == len(faces) > 0
        assert np.array_equal(o["vertices"][:nv], verts.astype(np.float32))

        def cyc(f):
            f = [int(x) for x in f]
            m = f.index(min(f))
            return tuple(f[m:] + f[:m])
        assert sorted(map(cyc, o["faces"][:nf])) == sorted(map(cyc, faces))


def test_the_table_in_the_source_is_the_rule():
    src = open(os.path.join(ROOT, "roma_amd", "csrc", "tsdf.hip")).read()

    def table(name):
        body = re.search(name + r"(?:\[\d+\])+ = \{(.*?)\};", src, re.S).group(1)
        return [int(x) for x in re.findall(r"\d+", body)]
    assert table("TET_NTRI") == tr.TET_NTRI
    assert table("TET_TRI") == [x for row in tr.TET_TRI for x in row]
    assert table("TET_CORNER") == [x for row in tr.TET_CORNER for x in row]
    assert table("TET_ODD") == tr.TET_ODD
    assert table("EDGE_END") == [x for row in tr.EDGE_END for x in row]
    # a positively oriented tetrahedron 0, x, y, z: every case's triangles point from the inside corners to the outside ones
    corner = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    for case in range(1, 15):
        ins = [n for n in range(4) if case >> n & 1]
        out = [n for n in range(4) if n not in ins]
        away = corner[out].mean(axis=0) - corner[ins].mean(axis=0)
        for n in range(tr.TET_NTRI[case]):
            P = np.array([corner[list(tr.EDGE_END[e])].mean(axis=0) for e in tr.TET_TRI[case][3 * n:3 * n + 3]])
            assert np.cross(P[1] - P[0], P[2] - P[0]) @ away > 0, case


# ------------------------------------------------------------------------------------------------------------- analytic fields
@pytest.mark.parametrize("kind,euler", [("sphere", 2), ("torus", 0)])
def test_analytic_fields_give_closed_oriented_surfaces(kind, euler):
    o = tc.field_ref(kind)
    nv, nf = (int(x) for x in o["counts"])
    assert tuple(o["totals"]) == (nv, nf) and nf == 2 * nv - 2 * euler and o["stats"][4] == 0 and o["stats"][5] == 0
    tc.check_topology(o["faces"][:nf], nv, euler)
    v = o["vertices"][:nv].astype(np.float64)
    tri = v[o["faces"][:nf]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.linalg.norm(n, axis=1) > 0).all()  # no face is degenerate in space either
    # the faces point outwards: the enclosed volume is positive, and within 5 % of the solid's
    volume = (tri.mean(axis=1) * n).sum() / 6.0
    true = 4.0 / 3.0 * math.pi * tc.SPHERE_R ** 3 if kind == "sphere" else 2.0 * math.pi ** 2 * tc.TORUS_R * tc.TORUS_r ** 2
    assert abs(volume / true - 1.0) < 0.05
    normals = o["normals"][:nv].astype(np.float64)
    finite = np.isfinite(normals).all(axis=1)
    # a normal is missing exactly where an end of the vertex's edge is in the outermost layer of the grid (the torus reaches it)
    assert np.array_equal(finite, ((v >= 1.0) & (v <= tc.FIELD_N - 2.0)).all(axis=1)) and finite.all() == (kind == "sphere")
    assert np.isnan(normals[~finite]).all() and np.abs(np.linalg.norm(normals[finite], axis=1) - 1.0).max() < 1e-6
    if kind == "sphere":
        pos, ang = tc.check_sphere_geometry(v, normals)
        print(f"sphere: vertices within {pos:.4f} cells (bound {tc.SPHERE_POS_BOUND:.4f}), normals within {ang:.4f} rad (bound {tc.SPHERE_NORMAL_BOUND:.4f})")
    else:
        # The tube's axis is 2.2 cells from the surface, nearer than an edge and a stencil reach (sqrt(3) + 1): the bound of the
        # sphere's derivation, 3 / rho^2 with rho the distance to that axis, is void here.  What holds without it: a vertex normal
        # lies within a right angle of the normal of every face around it.
        fn = n / np.linalg.norm(n, axis=1, keepdims=True)
        for corner in range(3):
            at = o["faces"][:nf, corner]
            assert ((normals[at] * fn).sum(axis=1)[finite[at]] > 0).all()


def test_open_mesh_cuts_and_empty_mesh_through_the_reference():
    full = tc.field_ref("sphere")
    o = tc.field_ref("sphere", slab=True)
    nv, nf = (int(x) for x in o["counts"])
    assert 0 < nv < full["counts"][0] and 0 < nf < full["counts"][1]
    used = np.zeros(nv, dtype=bool)
    used[o["faces"][:nf].reshape(-1)] = True
    assert o["stats"][4] == (~used).sum() > 0 and np.isnan(o["normals"][:nv]).any()
    per_edge = np.unique(np.sort(np.concatenate([o["faces"][:nf][:, [0, 1]], o["faces"][:nf][:, [1, 2]], o["faces"][:nf][:, [2, 0]]]), axis=1), axis=0,
                         return_counts=True)[1]
    assert per_edge.max() == 2 and (per_edge == 1).sum() > 0  # open: boundary edges
    tv, tf = (int(x) for x in full["totals"])
    cut = tc.field_ref("sphere", max_vertices=tv - 100, max_faces=tf - 50)
    assert tuple(cut["counts"]) == (tv - 100, tf - 50) and tuple(cut["totals"]) == (tv, tf)
    assert np.array_equal(cut["vertices"], full["vertices"][:tv - 100])
    bad = (full["faces"][:tf - 50] >= tv - 100).any(axis=1)
    assert cut["stats"][5] == bad.sum() > 0 and (cut["faces"][bad] == -1).all() and np.array_equal(cut["faces"][~bad], full["faces"][:tf - 50][~bad])
    none = tc.field_ref("sphere", min_weight=2.0)
    assert not none["counts"].any() and not none["totals"].any() and not none["stats"].any()
    assert np.isnan(none["vertices"]).all() and (none["faces"] == -1).all()


def test_chain_through_the_restatements():
    """depth_fusion_cases.chain_case through the restatements of every step - fused depth maps, bounds, volume, integration with
    colours, extraction - and a z-buffer over the vertices: the margins that the GPU file holds the device chain to"""
    from depth_fusion_cases import CHAIN_SIZES, chain_case, chain_ref_default
    c, fused = chain_case(), chain_ref_default()
    H, W, V = c["H"], c["W"], c["V"]
    origin, vs = tr.volume_from_bounds(tr.points_bounds(fused["points"], fused["count"]), tc.CHAIN_DIMS, 0.05)
    g = np.random.default_rng(5)
    images = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in CHAIN_SIZES]
    m = {}
    state = tr.integrate(*tr.fresh(tc.CHAIN_DIMS, True), fused["depth"], c["K_grid_exact"], c["R"], c["t"], origin, vs, tc.CHAIN_TRUNC_VOXELS * vs,
                         depth_weight=fused["weight"], images=images, near=1e-6, margins=m)
    mesh = tr.extract_mesh(*state, origin, vs, min_weight=float(np.finfo(np.float32).tiny), margins=m)
    nv, nf = (int(x) for x in mesh["counts"])
    assert nv > 2000 and tuple(mesh["totals"]) == (nv, nf) and mesh["colors"][:nv].max() > 0
    X = mesh["vertices"][:nv].astype(np.float64)
    y = X @ c["R"][0].T + c["t"][0]
    Kg = c["K_grid_exact"][0]
    col, row = np.floor(Kg[0, 0] * y[:, 0] / y[:, 2] + Kg[0, 2]).astype(int), np.floor(Kg[1, 1] * y[:, 1] / y[:, 2] + Kg[1, 2]).astype(int)
    zr = np.full((H, W), np.inf)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            r, q = row + dr, col + dc
            ok = (r >= 0) & (r < H) & (q >= 0) & (q < W) & (y[:, 2] > 0)
            np.minimum.at(zr, (r[ok], q[ok]), y[ok, 2].astype(np.float32))
    tc.check_chain(c, fused["depth"], vs, X, np.where(np.isfinite(zr), zr, np.nan))


def test_bounds_against_numpy():
    g = np.random.default_rng(4)
    pts = (g.normal(size=(500, 3)) * [3.0, 1.0, 0.2] + [100.0, -5.0, 0.0]).astype(np.float32)
    pts[g.random(500) < 0.2] = np.nan
    pts[7, 1] = np.inf
    pts[450:] *= 50.0  # beyond the count
    b = tr.points_bounds(pts, 450)
    rows = pts[:450][np.isfinite(pts[:450]).all(axis=1)].astype(np.float64)
    assert np.array_equal(b, np.stack([rows.min(axis=0), rows.max(axis=0)]))
    assert np.isnan(tr.points_bounds(pts, 0)).all() and np.isnan(tr.points_bounds(np.full((4, 3), np.nan))).all()
    signed = tr.points_bounds(np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, -1.0]], dtype=np.float32))
    assert np.signbit(signed[0, :2]).all() and not np.signbit(signed[1, :2]).any()
    # the volume around the box: cubic voxels, the box centred and inside with the margin
    from roma_amd.tsdf import volume_from_bounds
    dims = (24, 20, 16)
    origin, vs = tr.volume_from_bounds(b, dims, 0.05)
    o_t, vs_t = volume_from_bounds(torch.from_numpy(b), dims, 0.05)
    assert np.allclose(o_t.numpy(), origin, rtol=0, atol=1e-12) and abs(float(vs_t) - vs) < 1e-15
    n = np.array([16, 20, 24])
    assert (origin <= b[0] - 0.05 * (b[1] - b[0]).max() + 1e-12).all() and (origin + n * vs >= b[1] + 0.05 * (b[1] - b[0]).max() - 1e-12).all()
    assert np.allclose(origin + 0.5 * n * vs, 0.5 * (b[0] + b[1]))


def test_write_ply_reads_back(tmp_path):
    from roma_amd.tsdf import Mesh, write_ply
    o = tc.field_ref("sphere", max_vertices=2100, max_faces=4300)  # the last faces name cut vertices: left out
    colors = (np.arange(2100 * 3) % 251).astype(np.uint8).reshape(2100, 3)
    mesh = Mesh(*(torch.from_numpy(x) for x in (o["vertices"], o["normals"], colors, o["faces"], o["counts"], o["totals"], o["stats"])))
    path = str(tmp_path / "sphere.ply")
    nv, nf = write_ply(path, mesh)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element")}
    props = [ln.split()[-1] for ln in lines if ln.startswith("property") and "list" not in ln]
    assert counts == {"vertex": nv, "face": nf} and props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    rows = np.frombuffer(body[:nv * 27], dtype=np.dtype([("f", "<f4", (6,)), ("c", "u1", (3,))]))
    tris = np.frombuffer(body[nv * 27:], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    want_v, want_f = int(o["counts"][0]), o["faces"][:int(o["counts"][1])]
    want_f = want_f[(want_f >= 0).all(axis=1)]
    assert nv == want_v and len(tris) == nf == len(want_f) < o["counts"][1] and (tris["n"] == 3).all()
    assert np.array_equal(rows["f"][:, :3], o["vertices"][:nv]) and np.array_equal(rows["f"][:, 3:], o["normals"][:nv], equal_nan=True)
    assert np.array_equal(rows["c"], colors[:nv]) and np.array_equal(tris["v"], want_f)


@pytest.mark.parametrize("name,margins", list(tc.gpu_margins()), ids=lambda x: x if isinstance(x, str) else "")
def test_no_gpu_case_has_a_decision_on_the_edge(name, margins):
    assert set(margins) <= set(tr.KINDS)
    for kind, m in margins.items():
        assert m > tc.EDGE, (name, kind, m)


# ------------------------------------------------------------------------------------------------------------ the C ABI, no GPU
def test_third_table_is_its_golden_and_the_other_two_are_untouched():
    gold = os.path.join(ROOT, "tests", "golden")
    golden = json.load(open(os.path.join(gold, "abi_signatures_tsdf.json")))
    got = abi_classes(_lib.TSDF)
    assert sorted(got) == sorted(golden) == sorted(NEW_SYMBOLS)
    for name in golden:
        assert got[name] == golden[name], name
    assert abi_classes(_lib.SIGNATURES) == json.load(open(os.path.join(gold, "abi_signatures.json"))) and len(_lib.SIGNATURES) == 120
    assert abi_classes(_lib.EXTENSIONS) == json.load(open(os.path.join(gold, "abi_signatures_registration.json")))
    assert not set(_lib.TSDF) & (set(_lib.SIGNATURES) | set(_lib.EXTENSIONS))
    header = open(os.path.join(ROOT, "include", "roma_hip_tsdf.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert set(re.findall(r"\b(roma_[a-z0-9_]+)\s*\(", code)) == set(NEW_SYMBOLS)
    for other in ("roma_hip.h", "roma_hip_registration.h"):
        assert not any(n in open(os.path.join(ROOT, "include", other)).read() for n in NEW_SYMBOLS)
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "tsdf.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "tsdf" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()
    src = open(os.path.join(ROOT, "roma_amd", "csrc", "tsdf.hip")).read()
    assert '#include "../../include/roma_hip_tsdf.h"' in src  # the compiler holds the definitions to the declarations
    assert "#pragma clang fp contract(off)" in src and '#include "workspace.h"' in src and "Workspace256" in src


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_both_libraries_export_every_declared_name(fmt):
    lib = _lib.load(fmt)  # binds every name of the three tables, AttributeError on a missing one
    for name, (res, args) in _lib.TSDF.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    ws = lib.roma_op_tsdf_extract_mesh_workspace
    assert ws(0, 8, 8, 8, 10) == 0 and ws(1, 0, 8, 8, 10) == 0 and ws(1, 8, 8, 8, -1) == 0 and ws(1, 1024, 1024, 1024, 10) == 0
    assert ws(1, 674, 674, 674, 10) > 0 and ws(1, 675, 675, 675, 10) == 0  # 7 nz ny nx below 2^31
    assert ws(8, 645, 645, 645, 10) > 0 and ws(9, 645, 645, 645, 10) == 0  # B nz ny nx below 2^31
    assert 0 < ws(1, 8, 8, 8, 100) < ws(1, 16, 16, 16, 100) < ws(2, 16, 16, 16, 100)
    assert ws(1, 16, 16, 16, 1100) - ws(1, 16, 16, 16, 100) >= 1000 * 4 and ws(1, 32, 32, 32, 0) >= 5 * 32 ** 3
    wb = lib.roma_op_points_bounds_workspace
    assert wb(0) == 0 and wb(65536) == 0 and 0 < wb(1) <= wb(64)


def test_every_call_site_passes_the_declared_number_of_arguments():
    files = []
    for d in ("roma_amd", "tools"):
        files += sorted(glob.glob(os.path.join(ROOT, d, "*.py")))
    bad, seen = [], set()
    for f in files:
        for node in ast.walk(ast.parse(open(f).read(), f)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in _lib.TSDF:
                if any(isinstance(a, ast.Starred) for a in node.args):
                    continue
                seen.add(node.func.attr)
                want = len(_lib.TSDF[node.func.attr][1])
                if len(node.args) != want or node.keywords:
                    bad.append(f"{os.path.relpath(f, ROOT)}:{node.lineno} {node.func.attr}: {len(node.args)} arguments, declared {want}")
    assert seen == set(NEW_SYMBOLS) and not bad, (bad, set(NEW_SYMBOLS) - seen)


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    off = (C_longlong * 6)(*range(6))
    size = (C_int * 12)(*([5] * 12))

    def integ(depth=p, B=2, V=3, H=9, W=13, nz=8, ny=8, nx=8, mw=64.0, near=0.0, tsdf=p, color=None, images=None, offs=None, sizes=None, trunc=p):
        return lib.roma_op_tsdf_integrate(depth, None, p, p, p, None, None, images, offs, sizes, p, p, trunc, B, V, H, W, nz, ny, nx, mw, near,
                                          tsdf, p, color, None)

    need = lib.roma_op_tsdf_extract_mesh_workspace(2, 8, 8, 8, 100)

    def mesh(tsdf=p, B=2, nz=8, ny=8, nx=8, mw=1.0, maxv=100, maxf=200, color=None, out_c=None, faces=p, ws=p, nws=need):
        return lib.roma_op_tsdf_extract_mesh(tsdf, p, color, None, p, p, B, nz, ny, nx, mw, maxv, maxf, p, p, out_c, faces, p, p, p, ws, nws, None)

    nb = lib.roma_op_points_bounds_workspace(2)

    def bounds(pts=p, B=2, N=10, out=p, ws=p, nws=nb):
        return lib.roma_op_points_bounds(pts, None, B, N, out, ws, nws, None)

    size_bad = (C_int * 12)(*([5] * 11 + [0]))
    cases = [(lambda: integ(depth=None), "tsdf_integrate: null pointer"), (lambda: integ(tsdf=None), "null pointer"), (lambda: integ(trunc=None), "null pointer"),
             (lambda: integ(V=0), "1 <= V <= 8"), (lambda: integ(V=9), "1 <= V <= 8"), (lambda: integ(B=-1), "B must lie"), (lambda: integ(B=65536), "B must lie"),
             (lambda: integ(H=0), "H and W"), (lambda: integ(nx=0), "nz, ny and nx"), (lambda: integ(mw=0.0), "max_weight"), (lambda: integ(mw=math.nan), "max_weight"),
             (lambda: integ(near=-1.0), "near"), (lambda: integ(near=math.nan), "near"), (lambda: integ(images=p), "go together"),
             (lambda: integ(images=p, offs=off, sizes=size), "color and the colour source"), (lambda: integ(color=p), "color and the colour source"),
             (lambda: integ(nz=1024, ny=1024, nx=1024), "2^31"), (lambda: integ(nz=675, ny=675, nx=675, B=1), "2^31"), (lambda: integ(H=30000, W=30000), "B * V * H * W"),
             (lambda: integ(color=p, images=p, offs=off, sizes=size, B=43), "must not exceed 128"),
             (lambda: integ(color=p, images=p, offs=off, sizes=size_bad), "image sizes must be positive"),
             (lambda: mesh(tsdf=None), "tsdf_extract_mesh: null pointer"), (lambda: mesh(faces=None), "null pointer"), (lambda: mesh(color=p), "go together"),
             (lambda: mesh(out_c=p), "go together"), (lambda: mesh(B=-1), "B must lie"), (lambda: mesh(nz=0), "nz, ny and nx"), (lambda: mesh(mw=0.0), "min_weight"),
             (lambda: mesh(mw=math.nan), "min_weight"), (lambda: mesh(maxv=-1), "must not be negative"), (lambda: mesh(maxf=-1), "must not be negative"),
             (lambda: mesh(nz=1024, ny=1024, nx=1024), "2^31"), (lambda: mesh(maxf=2 ** 29), "3 * B * max_vertices"), (lambda: mesh(ws=None), "workspace too small"),
             (lambda: mesh(nws=need - 1), "workspace too small"), (lambda: mesh(nws=-5), "workspace too small"),
             (lambda: bounds(out=None), "points_bounds: null pointer"), (lambda: bounds(pts=None), "null pointer"), (lambda: bounds(B=-1), "B must lie"),
             (lambda: bounds(N=-1), "N must not be negative"), (lambda: bounds(B=4, N=2 ** 28), "3 * B * N"), (lambda: bounds(ws=None), "workspace too small"),
             (lambda: bounds(nws=nb - 1), "workspace too small")]
    for k, (call, word) in enumerate(cases):
        assert call() != 0 and word in lib.roma_last_error().decode(), (k, word, lib.roma_last_error())
    assert integ(B=0) == 0 and mesh(B=0) == 0 and bounds(B=0) == 0  # nothing to do, nothing touched


def test_python_functions_check_arguments_and_refuse_host_tensors(built_lib):
    import roma_amd
    from roma_amd._lib import RomaHipError
    from roma_amd.tsdf import Mesh, TSDFVolume
    z3, one = torch.zeros(3, dtype=torch.float64), torch.ones((), dtype=torch.float64)
    host = TSDFVolume(torch.ones(4, 4, 4), torch.zeros(4, 4, 4), None, z3, one, one)
    calls = [lambda: roma_amd.tsdf_volume((4, 4, 4), z3, one, one), lambda: roma_amd.points_bounds(torch.zeros(8, 3)),
             lambda: roma_amd.tsdf_bounds(torch.zeros(8, 3), None, (4, 4, 4)),
             lambda: roma_amd.integrate_depth_maps(host, torch.ones(2, 5, 5), torch.eye(3), torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3)),
             lambda: roma_amd.extract_mesh(host)]
    for call in calls:
        with pytest.raises(RomaHipError, match=r"roma_amd\.tsdf: .* must be a tensor on a HIP device; there is no CPU fallback"):
            call()
    for bad in ((4, 4), (4, 0, 4), (4.5, 4, 4), (1024, 1024, 1024)):
        with pytest.raises(ValueError, match="roma_amd.tsdf: "):
            roma_amd.tsdf_volume(bad, z3, one, one)
    with pytest.raises(ValueError, match="must be a TSDFVolume"):
        roma_amd.extract_mesh((host.tsdf, host.weight))
    with pytest.raises(ValueError, match="DenseFusion"):
        roma_amd.mesh_from_fusion(None, None, None, None)
    with pytest.raises(ValueError, match="one Mesh without a batch axis"):
        roma_amd.write_ply("x.ply", Mesh(*(torch.zeros(2, 3, 3),) * 7))
    for name in ("TSDFVolume", "Mesh", "tsdf_volume", "tsdf_bounds", "points_bounds", "integrate_depth_maps", "extract_mesh", "mesh_from_fusion", "write_ply"):
        assert name in roma_amd.__all__ and hasattr(roma_amd, name)
    assert TSDFVolume._fields == ("tsdf", "weight", "color", "origin", "voxel_size", "trunc")
    assert Mesh._fields == ("vertices", "normals", "colors", "faces", "counts", "totals", "stats")
    assert roma_amd.tsdf.default_mesh_sizes((24, 20, 16)) == (16 * (16 * 20 + 20 * 24 + 16 * 24), 32 * (16 * 20 + 20 * 24 + 16 * 24))
    assert hasattr(roma_amd.RegressionMatcher, "mesh_image_set")


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_tsdf_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "tsdf.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/tsdf.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::|<.*", "", k["name"]) for k in ks)
    assert names == ["mesh_count_kernel", "mesh_face_kernel", "mesh_scan_kernel", "mesh_vertex_kernel", "points_bounds_kernel",
                     "tsdf_integrate_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] <= 64, k  # eight waves a SIMD: the sweeps hide their loads by occupancy
