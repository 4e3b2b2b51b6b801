"""Device TSDF fusion and mesh extraction (roma_amd.tsdf; csrc/tsdf.hip) against the numpy restatement tools/tsdf_ref.py: every
comparison exact, the floats by their int32 bits, unless stated; then the chain - the fused depth maps of `fuse_image_set` to a
mesh - and two reconstructions in two gauges integrated into one volume.  test_cpu_tsdf.py asserts that no decision of any case
compared here lies within 1e-9 of its threshold."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_cases as tc
from depth_fusion_cases import CHAIN_SIZES, chain_case
from tsdf_cases import tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MESH_KEYS = ("vertices", "normals", "colors", "faces", "counts", "totals", "stats")


def _dev(x, dtype):
    return None if x is None else torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _bits(x):
    """float32 as int32 bits with one NaN pattern, everything else unchanged"""
    x = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    if x.dtype != np.float32:
        return x
    return np.where(np.isnan(x), np.int32(0x7fc00000), x.view(np.int32))


def _same(a, b, where=""):
    if b is None:
        assert a is None, where
        return
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (where, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (where, int((a != b).sum()))


def _volume(cases, color=None):
    """a fresh batched volume for a list of cases on one grid (a single case: no batch axis)"""
    from roma_amd import tsdf_volume
    single = isinstance(cases, dict)
    cs = [cases] if single else cases
    color = cs[0]["images"] is not None if color is None else color
    origin = _dev([c["origin"] for c in cs], np.float64)
    vs, trunc = _dev([c["voxel_size"] for c in cs], np.float64), _dev([c["trunc"] for c in cs], np.float64)
    if single:
        origin, vs, trunc = origin[0], vs[0], trunc[0]
    return tsdf_volume(cs[0]["dims"], origin, vs, trunc, color=color)


def _integrate(vol, c, views=None, **kw):
    from roma_amd import integrate_depth_maps
    sel = list(range(len(c["depth"]))) if views is None else list(views)
    images = None if c["images"] is None or vol.color is None else [_dev(c["images"][v], np.uint8) for v in sel]
    vv = None if c["view_valid"] is None else [c["view_valid"][v] for v in sel]
    return integrate_depth_maps(vol, _dev(c["depth"][sel], np.float32), _dev(c["K"][sel], np.float64), _dev(c["R"][sel], np.float64),
                                _dev(c["t"][sel], np.float64), depth_weight=None if c["depth_weight"] is None else _dev(c["depth_weight"][sel], np.float32),
                                images=images, view_valid=vv, max_weight=kw.get("max_weight", c["max_weight"]), near=c["near"])


def _state_same(vol, ref, where=""):
    _same(vol.tsdf, ref[0], (where, "tsdf"))
    _same(vol.weight, ref[1], (where, "weight"))
    _same(vol.color, ref[2], (where, "color"))


def _mesh_same(mesh, o, where=""):
    for k, x in zip(MESH_KEYS, mesh):
        _same(x, o[k], (where, k))


def _field_volume(kind, n=tc.FIELD_N, weight=None):
    from roma_amd import TSDFVolume
    tsdf, w = tc.field(kind, n)
    one = torch.ones((), device=DEV, dtype=torch.float64)
    return TSDFVolume(_dev(tsdf, np.float32), _dev(w if weight is None else weight, np.float32), None, _dev(tc.FIELD_ORIGIN, np.float64), one,
                      one * tc.FIELD_TRUNC)


def test_hand_made(built_lib):
    from roma_amd import extract_mesh
    c = tc.hand_made()
    vol = _integrate(_volume(c), c)
    mesh = extract_mesh(vol, min_weight=0.5)
    tc.check_hand_made(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), {k: None if x is None else x.cpu().numpy() for k, x in zip(MESH_KEYS, mesh)})
    ref = tc.run_ref(c)
    _state_same(vol, ref)
    _mesh_same(mesh, tr.extract_mesh(ref[0], ref[1], None, c["origin"], c["voxel_size"], min_weight=0.5))


@pytest.mark.parametrize("weights,colors,max_weight", tc.SMALL_VARIANTS)
def test_small_integration_against_the_restatement(built_lib, weights, colors, max_weight):
    """V = 3 views of 24 x 32 into 24 x 20 x 16 (30 blocks): with and without depth_weight and colours, max_weight reached"""
    c = tc.small_case(weights, colors)
    ref, _ = tc.small_ref(weights, colors, max_weight)
    vol = _integrate(_volume(c), c, max_weight=max_weight)
    _state_same(vol, ref)
    assert (ref[1] == np.float32(max_weight)).any() == (max_weight < 3.0) and 0 < (ref[1] > 0).mean() < 1


def test_large_integration_in_one_call_in_two_and_in_eight(built_lib):
    """V = 8 views of 48 x 64 into 96 x 80 x 64 (1 920 blocks): all views in one call, 4 + 4 and 8 single-view calls give the
    restatement's bits"""
    c = tc.large_case()
    ref, _ = tc.large_ref()
    one = _integrate(_volume(c), c)
    _state_same(one, ref, "8")
    two = _volume(c)
    for part in ((0, 1, 2, 3), (4, 5, 6, 7)):
        _integrate(two, c, part)
    _state_same(two, ref, "4 + 4")
    eight = _volume(c)
    for v in range(8):
        _integrate(eight, c, (v,))
    _state_same(eight, ref, "8 x 1")


def test_far_origin_and_view_valid(built_lib):
    """the same scene moved by (1e3, -2e3, 5e2) with its cameras and its volume, view 2 not valid"""
    c = tc.large_case(far=True)
    ref, _ = tc.large_ref(far=True)
    vol = _integrate(_volume(c), c)
    _state_same(vol, ref)
    near = tc.large_ref()[0]  # the scene at the origin, every view: view 2 made a difference
    assert not np.array_equal(ref[1], near[1])


@pytest.mark.parametrize("kind,euler", [("sphere", 2), ("torus", 0)])
def test_analytic_fields_on_the_device(built_lib, kind, euler):
    from roma_amd import extract_mesh
    mesh = extract_mesh(_field_volume(kind), min_weight=0.5)
    _mesh_same(mesh, tc.field_ref(kind), kind)
    nv, nf = (int(x) for x in mesh.counts.cpu())
    tc.check_topology(mesh.faces[:nf].cpu().numpy(), nv, euler)
    assert nf == 2 * nv - 2 * euler and int(mesh.stats[4]) == 0
    if kind == "sphere":
        tc.check_sphere_geometry(mesh.vertices[:nv].cpu().numpy(), mesh.normals[:nv].cpu().numpy())


def test_sphere_over_many_blocks_of_the_scan(built_lib):
    """96^3: 3 456 blocks, more than the 1 024 threads of the scan's workgroup, so every thread walks several"""
    from roma_amd import extract_mesh
    mesh = extract_mesh(_field_volume("sphere", 96), min_weight=0.5)
    o = tc.field_ref("sphere", 96)
    _mesh_same(mesh, o)
    assert o["counts"][0] > 40000 and tuple(o["counts"]) == tuple(o["totals"])
    again = extract_mesh(_field_volume("sphere", 96), min_weight=0.5)
    assert all(a is None and b is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(mesh, again))


def test_open_mesh_empty_mesh_and_cuts(built_lib):
    from roma_amd import extract_mesh
    o = tc.field_ref("sphere", slab=True)
    tsdf, w = tc.field("sphere")
    k, i = np.meshgrid(np.arange(tc.FIELD_N), np.arange(tc.FIELD_N), indexing="ij")
    w = w.copy()
    w[:, tc.SLAB[0]:tc.SLAB[1], :] *= ((i + 2 * k) % 3 == 0)[:, None, :]
    mesh = extract_mesh(_field_volume("sphere", weight=w), min_weight=0.5)
    _mesh_same(mesh, o, "slab")
    assert int(mesh.stats[4]) == o["stats"][4] > 0
    none = extract_mesh(_field_volume("sphere"), min_weight=2.0)
    _mesh_same(none, tc.field_ref("sphere", min_weight=2.0), "empty")
    assert not none.counts.any() and bool(torch.isnan(none.vertices).all()) and bool((none.faces == -1).all())
    tv, tf = (int(x) for x in tc.field_ref("sphere")["totals"])
    for mv, mf in ((tv - 100, None), (None, tf - 50), (tv - 100, tf - 50), (1, 1)):
        cut = extract_mesh(_field_volume("sphere"), min_weight=0.5, max_vertices=tv if mv is None else mv, max_faces=tf if mf is None else mf)
        ref = tc.field_ref("sphere", max_vertices=tv if mv is None else mv, max_faces=tf if mf is None else mf)
        _mesh_same(cut, ref, (mv, mf))
        assert tuple(cut.totals.cpu().numpy()) == (tv, tf)
    assert ref["stats"][5] == 1  # the one face written names a vertex that was not


def test_ragged_batch_single_calls_second_run_and_permutation(built_lib):
    from roma_amd import extract_mesh
    cases, refs = tc.ragged_batch(), tc.ragged_refs()

    def run(order):
        cs = [cases[b] for b in order]
        vol = _volume(cs)
        from roma_amd import integrate_depth_maps
        integrate_depth_maps(vol, _dev(np.stack([c["depth"] for c in cs]), np.float32), _dev(np.stack([c["K"] for c in cs]), np.float64),
                             _dev(np.stack([c["R"] for c in cs]), np.float64), _dev(np.stack([c["t"] for c in cs]), np.float64),
                             depth_weight=_dev(np.stack([c["depth_weight"] for c in cs]), np.float32), valid=[tc.RAGGED_VALID[b] for b in order])
        return vol, extract_mesh(vol, min_weight=0.1, valid=[tc.RAGGED_VALID[b] for b in order])
    vol, mesh = run((0, 1, 2))
    for b, (state, o, _) in enumerate(refs):
        _state_same(type(vol)(*(None if x is None else x[b] for x in vol)), state, b)
        _mesh_same([None if x is None else x[b] for x in mesh], o, b)
    assert refs[0][1]["counts"][0] > 100 and not refs[1][1]["counts"].any() and not refs[2][1]["counts"].any()
    vol2, mesh2 = run((0, 1, 2))
    vol3, mesh3 = run((2, 0, 1))
    for x, y, z in zip(list(vol[:2]) + [m for m in mesh if m is not None], list(vol2[:2]) + [m for m in mesh2 if m is not None],
                       list(vol3[:2]) + [m for m in mesh3 if m is not None]):
        _same(x, y.cpu().numpy(), "second run")
        _same(x[[2, 0, 1]], z.cpu().numpy(), "permuted")
    c = cases[0]  # and the single-problem form
    single = _integrate(_volume(c), c)
    _state_same(single, refs[0][0], "single")
    _mesh_same(extract_mesh(single, min_weight=0.1), refs[0][1], "single")


def _guarded(shape, dtype, poison):
    """a tensor inside a poisoned buffer with 256 bytes of guard on both sides"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 512,), 0xA5, device=DEV, dtype=torch.uint8)
    view = buf[256:256 + n].view(dtype).reshape(shape)
    view.fill_(poison)
    return buf, view


def _bands_intact(bufs):
    return all(bool((b[:256] == 0xA5).all()) and bool((b[-256:] == 0xA5).all()) for b in bufs)


def test_workspace_content_does_not_matter_and_nothing_is_written_outside(built_lib):
    lib = built_lib
    p = lambda x: C.c_void_p(x.data_ptr() if x is not None else 0)  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    # integration: the state inside guard bands
    c = tc.small_case(True, True)
    ref, _ = tc.small_ref(True, True, 64.0)
    nz, ny, nx = c["dims"]
    (bt, T), (bw, Wt), (bc, Cl) = _guarded((nz, ny, nx), torch.float32, 1.0), _guarded((nz, ny, nx), torch.float32, 0.0), _guarded((nz, ny, nx, 3), torch.float32, 0.0)
    images = [_dev(im, np.uint8) for im in c["images"]]
    packed = torch.cat([im.reshape(-1) for im in images])
    sizes = np.asarray([im.shape[:2] for im in c["images"]], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum([im.size for im in c["images"]])[:-1]]).astype(np.int64)
    depth, dw, K, R, t = (_dev(c[k], d) for k, d in (("depth", np.float32), ("depth_weight", np.float32), ("K", np.float64), ("R", np.float64), ("t", np.float64)))
    origin, vs, trunc = _dev(c["origin"], np.float64), _dev([c["voxel_size"]], np.float64), _dev([c["trunc"]], np.float64)
    rc = lib.roma_op_tsdf_integrate(p(depth), p(dw), p(K), p(R), p(t), None, None, p(packed), offs.ctypes.data, sizes.ctypes.data, p(origin), p(vs), p(trunc),
                                    1, 3, 24, 32, nz, ny, nx, 64.0, 1e-6, p(T), p(Wt), p(Cl), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.roma_last_error()
    assert _bands_intact([bt, bw, bc])
    _same(T, ref[0]), _same(Wt, ref[1]), _same(Cl, ref[2])
    # extraction: every output and the workspace inside guard bands, the workspace pre-filled
    tv, tf = (int(x) for x in tr.extract_mesh(ref[0], ref[1], ref[2], c["origin"], c["voxel_size"], min_weight=0.1)["totals"])
    MV, MF = tv + 50, tf - 30  # padding after the vertices, a cut in the faces
    o = tr.extract_mesh(ref[0], ref[1], ref[2], c["origin"], c["voxel_size"], min_weight=0.1, max_vertices=MV, max_faces=MF)
    assert tv > 100 and tf > 100
    nws = int(lib.roma_op_tsdf_extract_mesh_workspace(1, nz, ny, nx, MV))
    for fill in (0xFF, 0x00):
        ws = torch.full((256 + nws + 256,), fill, device=DEV, dtype=torch.uint8)
        ws[:256], ws[256 + nws:] = 0x5A, 0x5A
        outs = [_guarded((MV, 3), torch.float32, -7.0), _guarded((MV, 3), torch.float32, -7.0), _guarded((MV, 3), torch.uint8, 0x77),
                _guarded((MF, 3), torch.int32, -7), _guarded((2,), torch.int32, -7), _guarded((2,), torch.int32, -7), _guarded((8,), torch.int32, -7)]
        rc = lib.roma_op_tsdf_extract_mesh(p(T), p(Wt), p(Cl), None, p(origin), p(vs), 1, nz, ny, nx, 0.1, MV, MF, *(p(v) for _, v in outs),
                                           C.c_void_p(ws[256:].data_ptr()), nws, stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.roma_last_error()
        assert bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nws:] == 0x5A).all()), "the band around the workspace"
        assert _bands_intact([b for b, _ in outs])
        _mesh_same([v for _, v in outs], o, fill)  # every element of every output is written: none keeps its poison
    # bounds: the same
    nb = int(lib.roma_op_points_bounds_workspace(1))
    pts = _dev(o["vertices"], np.float32)
    for fill in (0xFF, 0x00):
        ws = torch.full((256 + nb + 256,), fill, device=DEV, dtype=torch.uint8)
        ws[:256], ws[256 + nb:] = 0x5A, 0x5A
        bo, out = _guarded((2, 3), torch.float64, -7.0)
        rc = lib.roma_op_points_bounds(p(pts), None, 1, MV, p(out), C.c_void_p(ws[256:].data_ptr()), nb, stream())
        torch.cuda.synchronize()
        assert rc == 0 and _bands_intact([bo]) and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nb:] == 0x5A).all())
        assert np.array_equal(out.cpu().numpy(), tr.points_bounds(o["vertices"]))


def test_points_bounds_and_the_volume_around_a_cloud(built_lib):
    from roma_amd import points_bounds, tsdf_bounds
    g = np.random.default_rng(8)
    pts = (g.normal(size=(3, 70001, 3)) * [3.0, 1.0, 0.2] + [100.0, -5.0, 0.0]).astype(np.float32)
    pts[g.random((3, 70001)) < 0.2] = np.nan
    pts[0, 7, 1], pts[1, 9, 2] = np.inf, -np.inf
    pts[:, 60000:] *= 50.0
    counts = [60000, 0, 70001]
    b = points_bounds(_dev(pts, np.float32), counts)
    want = np.stack([tr.points_bounds(pts[k], counts[k]) for k in range(3)])
    assert np.array_equal(b.cpu().numpy(), want, equal_nan=True) and np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()
    assert np.array_equal(points_bounds(_dev(pts[2], np.float32)).cpu().numpy(), want[2])
    assert np.array_equal(b.cpu().numpy(), points_bounds(_dev(pts, np.float32), counts).cpu().numpy(), equal_nan=True)
    origin, vs = tsdf_bounds(_dev(pts, np.float32), _dev(counts, np.int32), (24, 20, 16), 0.05)
    for k in (0, 2):
        o_ref, vs_ref = tr.volume_from_bounds(want[k], (24, 20, 16), 0.05)
        assert np.allclose(origin[k].cpu().numpy(), o_ref, rtol=0, atol=1e-12) and abs(float(vs[k]) - vs_ref) < 1e-15
    assert bool(torch.isnan(vs[1]))  # a problem without a point gives a volume that every operator leaves alone


def _matcher(weights0, **kw):
    from roma_amd import roma_model
    sd, dsd = weights0
    return roma_model((112, 112), True, device=DEV, weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                      upsample_res=(168, 168), **kw)


def test_chain_fused_depth_maps_to_a_coloured_mesh(built_lib, weights0, tmp_path):
    """`mesh_image_set` on the ground-truth warps of four views, with colours; the vertices against the two planes and the mesh
    rendered through its vertices into view 0 against the fused depth, both under the margins that tsdf_cases.check_chain derives"""
    from roma_amd import render_points, write_ply
    c = chain_case()
    model = _matcher(weights0, max_batch=1)
    g = np.random.default_rng(5)
    images = [_dev(g.integers(0, 256, (h, w, 3), dtype=np.uint8), np.uint8) for h, w in CHAIN_SIZES]
    R, t = _dev(c["R"], np.float64), _dev(c["t"], np.float64)
    mesh, vol, fused = model.mesh_image_set(_dev(c["warp"], np.float32), _dev(c["certainty"], np.float32), c["pairs"], c["K"], R, t, c["sizes"],
                                            images=images, min_certainty=0.5, mesh=dict(dims=tc.CHAIN_DIMS, trunc_voxels=tc.CHAIN_TRUNC_VOXELS))
    H, W = c["H"], c["W"]
    nv, nf = (int(x) for x in mesh.counts.cpu())
    assert nv > 2000 and nf > 2000 and tuple(mesh.totals.cpu().numpy()) == (nv, nf) and mesh.colors is not None and vol.color is not None
    faces = mesh.faces[:nf].cpu().numpy()
    assert faces.min() >= 0 and faces.max() < nv and int(mesh.stats[5]) == 0
    back = render_points(mesh.vertices, c["K_grid_exact"][0], R[:1], t[:1], H, W, counts=mesh.counts[:1], radius=1, occlusion_radius=0, fill_radius=0)
    tc.check_chain(c, fused.depth.cpu().numpy(), float(vol.voxel_size), mesh.vertices[:nv].cpu().numpy(), back.depth[0].cpu().numpy())
    # the colours come from the images, and the file holds what the counts say
    assert int(mesh.colors[:nv].max()) > 0 and int(mesh.colors[nv:].max() if nv < mesh.colors.shape[0] else 0) == 0
    assert write_ply(str(tmp_path / "chain.ply"), mesh) == (nv, nf)


def test_two_gauges_twelve_views_in_one_volume(built_lib):
    """Six views in the gauge of the volume and six of a second reconstruction whose gauge is a similarity away: its cameras come
    back through `apply_similarity` with the inverse, its depths divided by the scale, and all twelve go into one volume in two
    calls - more views than any one operator takes.  The device's moved cameras and depths then go through the restatement."""
    from roma_amd import apply_similarity, extract_mesh
    a = tc.scene_case(6, 24, 32, tc.SMALL_DIMS, tc.GAUGE_SEED, colors=False)
    b = tc.scene_case(6, 24, 32, tc.SMALL_DIMS, tc.GAUGE_SEED + 1, colors=False, phase=0.5)
    g = np.random.default_rng(tc.GAUGE_SEED)
    s = 1.7
    q, _ = np.linalg.qr(g.normal(size=(3, 3)))
    Rs = q * np.sign(np.linalg.det(q))
    ts = g.uniform(-2, 2, 3)
    # the second reconstruction as it would come: cameras and depths in ITS gauge, X2 = s Rs X + ts
    R2 = b["R"] @ Rs.T
    t2 = s * b["t"] - R2 @ ts
    depth2 = (b["depth"].astype(np.float64) * s).astype(np.float32)
    inv = (_dev(1.0 / s, np.float64), _dev(Rs.T, np.float64), _dev(-Rs.T @ ts / s, np.float64))
    Rb, tb = apply_similarity(inv, R=_dev(R2, np.float64), t=_dev(t2, np.float64))
    depth_b = _dev(depth2, np.float32) / np.float32(s)
    assert np.abs(Rb.cpu().numpy() - b["R"]).max() < 1e-12 and np.abs(tb.cpu().numpy() - b["t"]).max() < 1e-12
    vol = _integrate(_volume(a), a)
    moved = dict(b, R=Rb.cpu().numpy(), t=tb.cpu().numpy(), depth=depth_b.cpu().numpy())
    _integrate(vol, moved)
    m = {}
    ref = tc.run_ref(moved, state=tc.run_ref(a, margins=m), margins=m)
    assert min(m.values()) > tc.EDGE
    _state_same(vol, ref)
    seen = tc.run_ref(dict(moved, depth_weight=None), state=tc.run_ref(dict(a, depth_weight=None)))[1]  # with weight 1 a view counts 1
    assert seen.max() > 8  # voxels that more than eight views saw
    mesh = extract_mesh(vol, min_weight=0.5)
    o = tr.extract_mesh(ref[0], ref[1], None, a["origin"], a["voxel_size"], min_weight=0.5)
    _mesh_same(mesh, o)
    nv = int(mesh.counts[0])
    assert nv > 300
