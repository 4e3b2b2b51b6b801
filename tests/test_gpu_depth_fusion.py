"""Device dense depth fusion (roma_amd.fuse_depth_maps, roma_amd.relative_poses; csrc/depth_fusion.hip) against the numpy restatement
tools/depth_fusion_ref.py: every comparison exact, the floats by their int32 bits; then the chain RegressionMatcher.fuse_image_set
on ground-truth warps against the chain of restatements, and dense_reconstruct_image_set against its manual composition.
test_cpu_depth_fusion.py asserts that no decision of any case compared here lies within 1e-9 of its threshold."""
import ctypes as C

import numpy as np
import pytest
import torch

from depth_fusion_cases import (CHAIN_SIZES, HAND_KW, RAGGED_VALID, RAGGED_VIEW_VALID, RANDOM_PARAMS, WIDE_CUT, chain_case, chain_ref_default,
                                check_hand_made, color_case, color_ref, dfr, hand_made, large_case, large_ref, ragged_batch, ragged_refs, random_case,
                                random_ref, ref, wide_case, wide_ref)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# DenseFusion's fields and the restatement's names for them
KEYS = ("depth", "weight", "support", "seen", "violated", "state", "points", "colors", "cloud_weight", "source", "count", "total", "stats")


def _dev(x, dtype):
    return None if x is None else torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _bits(x):
    """float32 as int32 bits with one NaN pattern, everything else unchanged"""
    x = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    if x.dtype != np.float32:
        return x
    return np.where(np.isnan(x), np.int32(0x7fc00000), x.view(np.int32))


def _args(c):
    return (_dev(c["points"], np.float32), _dev(c["flags"], np.uint8), _dev(c["certainty"], np.float32), c["pairs"], _dev(c["cameras"], np.float64),
            _dev(c["R"], np.float64), _dev(c["t"], np.float64))


def _run(c, **kw):
    from roma_amd import fuse_depth_maps
    kw.setdefault("symmetric", c["symmetric"])
    return fuse_depth_maps(*_args(c), **kw)


def _as_dict(d):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in zip(KEYS, d)}


def _same_as_ref(d, o, where=""):
    """every output equals the restatement's, the floats bit for bit"""
    d = _as_dict(d) if not isinstance(d, dict) else d
    for k in KEYS:
        if o[k] is None:
            assert d[k] is None, (where, k)
            continue
        a, b = np.asarray(d[k]), np.asarray(o[k])
        assert a.shape == b.shape, (where, k, a.shape, b.shape)
        assert np.array_equal(_bits(a), _bits(b.astype(a.dtype) if b.dtype.kind in "iu" else b)), (where, k)


def test_hand_made(built_lib):
    c = hand_made()
    for dedupe in (True, False):
        kw = dict(HAND_KW, dedupe=dedupe)
        d = _run(c, max_points=4, **kw)
        check_hand_made(_as_dict(d), dedupe)
        _same_as_ref(d, ref(c, max_points=4, **kw), dedupe)


@pytest.mark.parametrize("rel,ms,mc,dd", RANDOM_PARAMS)
def test_random_against_the_restatement(built_lib, rel, ms, mc, dd):
    """V = 4, 24 x 40, six pairs - one reversed, one in both orders; 0.5 % noise, 10 % outlier slots, 5 % flagged, half the certainties 1"""
    o = random_ref(rel, ms, mc, dd)
    d = _run(random_case(), rel_thresh=rel, min_support=ms, min_consistent=mc, dedupe=bool(dd))
    _same_as_ref(d, o, (rel, ms, mc, dd))
    assert o["stats"][1] > 1000 and o["total"] > 0 and (o["stats"][3] > 0) == bool(dd)
    n = o["count"]  # the padding beyond the cloud
    assert np.isnan(d.points[n:].cpu().numpy()).all() and bool((d.source[n:] == -1).all()) and not bool(d.cloud_weight[n:].any())


def test_random_without_certainty_and_not_symmetric(built_lib):
    d = _run(random_case(True, False), rel_thresh=0.01, min_support=2, min_consistent=1, dedupe=True)
    _same_as_ref(d, random_ref(0.01, 2, 1, 1, True, False), "certainty None")
    d = _run(random_case(False, True), rel_thresh=0.01, min_support=2, min_consistent=1, dedupe=True)
    _same_as_ref(d, random_ref(0.01, 2, 1, 1, False, True), "symmetric 0")


def test_large_grid_scan_crosses_many_workgroups_and_the_cut(built_lib):
    """V = 3 at 160 x 200: 375 blocks of pixels; then max_points below total: the cut, the padding and total"""
    c, o = large_case(), large_ref()
    _same_as_ref(_run(c), o)
    assert o["total"] > 5000 and o["source"][0, 0] == 0 and o["source"][o["count"] - 1, 0] == 2
    cut = 3000
    oc = large_ref(cut)
    d = _run(c, max_points=cut)
    _same_as_ref(d, oc, "cut")
    assert int(d.total) == o["total"] > cut and int(d.counts) == cut and int(d.stats[4]) == cut
    assert np.array_equal(d.source.cpu().numpy(), o["source"][:cut]) and np.isfinite(d.points.cpu().numpy()).all()
    d = _run(c, max_points=o["total"] + 77)
    n = o["total"]
    assert int(d.counts) == n and np.isnan(d.points[n:].cpu().numpy()).all() and bool((d.source[n:] == -1).all())
    assert np.array_equal(_bits(d.points[:n]), _bits(o["points"][:n]))


def test_scan_threads_take_two_block_counts_each(built_lib):
    """V = 8 at 184 x 180: 1040 blocks of pixels for the 1024 threads of the scan kernel - two block counts a thread, none for the
    last 504 threads; then max_points below total"""
    c, o = wide_case(), wide_ref()
    _same_as_ref(_run(c, min_support=1), o)
    views = o["source"][:o["count"], 0]
    assert o["total"] > WIDE_CUT and (views == 0).any() and (views == 7).any()
    d = _run(c, min_support=1, max_points=WIDE_CUT)
    _same_as_ref(d, wide_ref(WIDE_CUT), "cut")
    assert int(d.total) == o["total"] and int(d.counts) == WIDE_CUT and np.array_equal(d.source.cpu().numpy(), o["source"][:WIDE_CUT])


def test_ragged_batch_equals_single_calls_and_runs_are_identical(built_lib):
    """a problem that is not valid, one with a view switched off, one without a usable slot"""
    from roma_amd import fuse_depth_maps
    cs, refs = ragged_batch(), ragged_refs()
    stack = lambda k, dt: _dev(np.stack([c[k] for c in cs]), dt)  # noqa: E731
    args = (stack("points", np.float32), stack("flags", np.uint8), stack("certainty", np.float32), cs[0]["pairs"], stack("cameras", np.float64),
            stack("R", np.float64), stack("t", np.float64))
    kw = dict(symmetric=True, min_support=1, valid=_dev(RAGGED_VALID, np.uint8), view_valid=_dev(RAGGED_VIEW_VALID, np.uint8))
    d = fuse_depth_maps(*args, **kw)
    again = fuse_depth_maps(*args, **kw)
    assert d.colors is None and again.colors is None
    for x, y in zip(d, again):
        assert x is None or np.array_equal(_bits(x), _bits(y))
    for b, c in enumerate(cs):
        one = _run(c, min_support=1, valid=_dev(RAGGED_VALID[b:b + 1], np.uint8), view_valid=_dev(RAGGED_VIEW_VALID[b], np.uint8))
        for k, x, y in zip(KEYS, d, one):
            assert x is None or np.array_equal(_bits(x[b]), _bits(y)), (b, k)
        _same_as_ref(one, refs[b], b)
    assert d.stats[0].cpu().tolist() == [0] * 8 and d.stats[2].cpu().tolist() == [0] * 8 and int(d.total[1]) > 0
    assert bool(torch.isnan(d.depth[0]).all()) and bool(torch.isnan(d.depth[1, 1]).all()) and not bool(d.support[2].any())
    assert not bool((d.seen[1] & 2).any()) and bool(d.seen[1].any())  # the view that is switched off supports nothing


def _guarded(shape, dtype, poison):
    """a tensor inside a poisoned buffer with 256 bytes of guard on both sides"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 512,), 0xA5, device=DEV, dtype=torch.uint8)
    view = buf[256:256 + n].view(dtype).reshape(shape)
    view.fill_(poison)
    return buf, view


def _raw(lib, c, fill, max_points, images=None, **kw):
    """the C entry on guarded outputs and a guarded workspace pre-filled with `fill`"""
    P, H, Wd = c["flags"].shape
    V, W = len(c["cameras"]), Wd // 2
    points, flags, cert, _, cam, R, t = _args(c)
    pv = np.ascontiguousarray(np.asarray(c["pairs"], np.int32))
    nws = int(lib.roma_op_fuse_depth_maps_workspace(1, V, H, W))
    ws = torch.full((256 + nws + 256,), fill, device=DEV, dtype=torch.uint8)
    ws[:256], ws[256 + nws:] = 0x5A, 0x5A
    f, u, i = torch.float32, torch.uint8, torch.int32
    K = max_points
    outs = [_guarded((V, H, W), f, -7.0), _guarded((V, H, W), f, -7.0)] + [_guarded((V, H, W), u, 0x77) for _ in range(4)]
    outs += [_guarded((K, 3), f, -7.0), _guarded((K, 3), u, 0x77) if images is not None else (None, None), _guarded((K,), f, -7.0),
             _guarded((K, 2), i, -7), _guarded((1,), i, -7), _guarded((1,), i, -7), _guarded((8,), i, -7)]
    p = lambda x: C.c_void_p(x.data_ptr() if x is not None else 0)  # noqa: E731
    packed = offsets = sizes = None
    if images is not None:
        packed = torch.cat([_dev(im, np.uint8).reshape(-1) for im in images])
        offsets = np.cumsum([0] + [im.size for im in images[:-1]]).astype(np.int64)
        sizes = np.ascontiguousarray(np.asarray([im.shape[:2] for im in images], np.int32))
    torch.cuda.synchronize()
    rc = lib.roma_op_fuse_depth_maps(p(points), p(flags), p(cert), pv.ctypes.data, p(cam), p(R), p(t), None, None, p(packed),
                                     offsets.ctypes.data if images is not None else None, sizes.ctypes.data if images is not None else None,
                                     1, V, P, H, W, 1, kw.get("rel_thresh", 0.01), kw.get("min_support", 2), kw.get("min_consistent", 1), 0, 1, K,
                                     *(p(v) for _, v in outs), C.c_void_p(ws[256:].data_ptr()), nws,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, lib.roma_last_error()
    assert bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nws:] == 0x5A).all()), "the band around the workspace"
    for k, (buf, _) in zip(KEYS, outs):
        assert buf is None or (bool((buf[:256] == 0xA5).all()) and bool((buf[-256:] == 0xA5).all())), k
    out = {k: (None if v is None else v.cpu().numpy()) for k, (_, v) in zip(KEYS, outs)}
    out["count"], out["total"] = out["count"][0], out["total"][0]
    return out


def test_workspace_content_does_not_matter_and_nothing_is_written_outside(built_lib):
    c = random_case()
    o = ref(c, max_points=1500)
    for fill in (0xFF, 0x00):
        _same_as_ref(_raw(built_lib, c, fill, 1500), o, fill)  # every element of every output is written: none keeps its poison
    cut = ref(c, max_points=100)
    _same_as_ref(_raw(built_lib, c, 0xFF, 100), cut, "cut")


def test_colours_of_two_images_of_different_sizes(built_lib):
    c, o = color_case(), color_ref()
    d = _run(c, min_support=1, images=[_dev(im, np.uint8) for im in c["images"]])
    _same_as_ref(d, o)
    n = o["count"]
    assert n > 100 and len(np.unique(o["colors"][:n], axis=0)) > 50 and not o["colors"][n:].any()
    _same_as_ref(_raw(built_lib, c, 0xFF, 2 * 20 * 28, images=c["images"], min_support=1), o, "raw")


def test_relative_poses(built_lib):
    from roma_amd import relative_poses
    c = random_case()
    Rij, tij = relative_poses(_dev(c["R"], np.float64), _dev(c["t"], np.float64), c["pairs"])
    Ro, to = dfr.relative_poses(c["R"], c["t"], c["pairs"])
    assert np.array_equal(Rij.cpu().numpy().view(np.int64), Ro.view(np.int64)) and np.array_equal(tij.cpu().numpy().view(np.int64), to.view(np.int64))
    Rb, tb = relative_poses(_dev(np.stack([c["R"]] * 3), np.float64), _dev(np.stack([c["t"]] * 3), np.float64), c["pairs"])
    assert tuple(Rb.shape) == (3, 6, 3, 3) and bool((Rb == Rij[None]).all()) and bool((tb == tij[None]).all())


def _matcher(weights0, **kw):
    from roma_amd import roma_model
    sd, dsd = weights0
    return roma_model((112, 112), True, device=DEV, weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                      upsample_res=(168, 168), **kw)


def _chain(model, c):
    return model.fuse_image_set(_dev(c["warp"], np.float32), _dev(c["certainty"], np.float32), c["pairs"], c["K"], _dev(c["R"], np.float64),
                                _dev(c["t"], np.float64), c["sizes"], min_certainty=0.5)


def test_chain_on_ground_truth_warps(built_lib, weights0):
    """fuse_image_set (K to the grid, relative_poses, one triangulate_warp call, fuse_depth_maps) on the ground-truth warps of four
    views of mixed image sizes equals the chain of restatements (triangulate_ref over the pairs, then depth_fusion_ref)"""
    from roma_amd import relative_poses, triangulate_warp
    c, o = chain_case(), chain_ref_default()
    d = _chain(_matcher(weights0, max_batch=1), c)
    # the link before the fusion, for a mismatch to name its stage: the depths of the one triangulate_warp call
    H, W = c["H"], c["W"]
    Kg = np.stack([c["K"][v] * np.array([[W / w], [H / h], [1.0]]) for v, (h, w) in enumerate(CHAIN_SIZES)])
    Rij, tij = relative_poses(_dev(c["R"], np.float64), _dev(c["t"], np.float64), c["pairs"])
    ia, ib = [i for i, _ in c["pairs"]], [j for _, j in c["pairs"]]
    tri = triangulate_warp(_dev(c["warp"], np.float32), _dev(c["certainty"], np.float32), Rij, tij, Kg[ia], Kg[ib], H, W, symmetric=True,
                           min_certainty=0.5)
    z = torch.cat((tri.depth_A, tri.depth_B), dim=2).cpu().numpy()
    f = torch.cat((tri.flags_A, tri.flags_B), dim=2).cpu().numpy()
    differ = int((_bits(z) != _bits(o["tri_points"][..., 2])).sum())
    print(f"triangulated depths that differ from the restatement's bits: {differ} of {z.size}; flags {int((f != o['tri_flags']).sum())}")
    assert np.array_equal(f, o["tri_flags"]) and differ == 0
    _same_as_ref(d, o)
    assert int(d.total) > 1000


def test_no_host_synchronisation(built_lib, weights0):
    c = chain_case()
    model = _matcher(weights0, max_batch=1)
    args = (_dev(c["warp"], np.float32), _dev(c["certainty"], np.float32), c["pairs"], _dev(c["K"], np.float64), _dev(c["R"], np.float64),
            _dev(c["t"], np.float64), c["sizes"])
    first = model.fuse_image_set(*args, min_certainty=0.5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = model.fuse_image_set(*args, min_certainty=0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for x, y in zip(first, again):
        assert x is None and y is None or np.array_equal(_bits(x), _bits(y))


def test_dense_reconstruct_image_set_is_its_manual_composition(built_lib, weights0):
    """Synthetic weights, three small images, coarse resolution 112.  The warps of random weights carry no geometry, so this
    checks only the plumbing: it runs, the shapes are right, it equals the manual composition bit for bit, the colours are the
    images', and 9 images are refused."""
    model = _matcher(weights0, max_batch=3)
    g = np.random.default_rng(5)
    sizes = [(120, 160), (96, 128), (150, 110)]
    ims = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    K = np.array([[[200.0, 0, w / 2], [0, 200.0, h / 2], [0, 0, 1]] for h, w in sizes])
    fusion = dict(rel_thresh=0.05, min_support=1, min_consistent=0, max_points=5000)
    fused, rec, tr, kp = model.dense_reconstruct_image_set(ims, K, 1e-3, 2.0, num=500, seed=7, max_kpts=1024, fusion=fusion)
    H, W = model.get_output_resolution()
    assert tuple(fused.depth.shape) == (3, H, W) and tuple(fused.points.shape) == (5000, 3) and tuple(fused.colors.shape) == (5000, 3)
    assert tuple(fused.stats.shape) == (8,) and tuple(rec.R.shape) == (3, 3, 3)
    rec2, tr2, kp2 = model.reconstruct_image_set(ims, K, 1e-3, 2.0, num=500, seed=7, max_kpts=1024)
    warp, cert, pairs = model.match_image_set(ims)
    fused2 = model.fuse_image_set(warp, cert, pairs, K, rec2.R, rec2.t, sizes, images=[_dev(im, np.uint8) for im in ims],
                                  view_valid=rec2.view_ok, **fusion)
    for a, b in zip((fused, rec, tr, kp), (fused2, rec2, tr2, kp2)):
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
    n, src, col = int(fused.counts), fused.source.cpu().numpy(), fused.colors.cpu().numpy()
    for k in range(0, n, max(1, n // 50)):  # the colour of a point is the image pixel under the centre of its cell
        v, q = src[k]
        r, c = divmod(int(q), W)
        assert np.array_equal(col[k], ims[v][((2 * r + 1) * sizes[v][0]) // (2 * H), ((2 * c + 1) * sizes[v][1]) // (2 * W)])
    with pytest.raises(ValueError, match="2 .. 8"):
        model.dense_reconstruct_image_set([ims[0]] * 9, K, 1e-3, 2.0)
