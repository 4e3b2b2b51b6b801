"""Device point-cloud rendering (roma_amd.render_points, roma_amd.orbit_cameras, RegressionMatcher.render_fusion;
csrc/point_render.hip) against the numpy restatement tools/point_render_ref.py: every comparison exact, the floats by their int32
bits; then the chain - the cloud `fuse_image_set` makes of ground-truth warps rendered back into its own views.
test_cpu_point_render.py asserts that no decision of any case compared here lies within 1e-9 of its threshold."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from depth_fusion_cases import CHAIN_SIZES, chain_case
from point_render_cases import (HAND_KW, RAGGED_COUNTS, RAGGED_VALID, RANDOM_PARAMS, check_hand_made, contention_case, contention_ref, hand_made,
                                large_case, large_ref, ragged_batch, ragged_refs, random_case, random_kw, random_ref, ref)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("color", "depth", "index", "mask", "stats")  # PointRender's fields, the restatement's names for them


def _dev(x, dtype):
    return None if x is None else torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _bits(x):
    """float32 as int32 bits with one NaN pattern, everything else unchanged"""
    x = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    if x.dtype != np.float32:
        return x
    return np.where(np.isnan(x), np.int32(0x7fc00000), x.view(np.int32))


def _run(c, cams=slice(None), **kw):
    from roma_amd import render_points
    count = None if c["count"] is None else _dev([c["count"]], np.int32)
    return render_points(_dev(c["points"], np.float32), _dev(c["cameras"][cams], np.float64), _dev(c["R"][cams], np.float64),
                         _dev(c["t"][cams], np.float64), c["H"], c["W"], colors=_dev(c["colors"], np.uint8), counts=count, **dict(c["kw"], **kw))


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
        assert a.shape == b.shape and a.dtype == b.dtype, (where, k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(_bits(a), _bits(b)), (where, k, int((_bits(a) != _bits(b)).sum()))


def _equal(x, y):
    return all(a is None and b is None or np.array_equal(_bits(a), _bits(b)) for a, b in zip(x, y))


def test_hand_made(built_lib):
    c = hand_made()
    d = _run(c)
    check_hand_made(_as_dict(d))
    _same_as_ref(d, ref(c))


@pytest.mark.parametrize("radius,flt,fil", RANDOM_PARAMS)
def test_random_against_the_restatement(built_lib, radius, flt, fil):
    """N = 20 000 (79 blocks of rows), C = 3, 48 x 64 (12 blocks of pixels): a sparse near surface in front of a dense far one"""
    _same_as_ref(_run(random_case(), **random_kw(radius, flt, fil)), random_ref(radius, flt, fil), (radius, flt, fil))


def test_a_frame_alone_equals_the_frame_among_three_and_runs_are_identical(built_lib):
    c, kw = random_case(), random_kw(1, "o2c3", "f1m3")
    d, again = _run(c, **kw), _run(c, **kw)
    assert _equal(d, again)
    for k in range(3):
        one = _run(c, cams=slice(k, k + 1), **kw)
        assert _equal([x[0] for x in one], [x[k] for x in d]), k


@pytest.mark.parametrize("radius", [0, 1])
def test_contention_in_one_pixel(built_lib, radius):
    """4 096 rows inside one pixel, 64 of them with the smallest float32 depth and none of those among the lowest rows: the tie rule
    and the early-out under the worst contention there is"""
    c, o = contention_case(), contention_ref(radius)
    d = _run(c, radius=radius)
    _same_as_ref(d, o, radius)
    r, col = 7, 9
    assert int(d.index[0, r, col]) == int(c["shared"][0]) > 200 and float(d.depth[0, r, col]) == 1.5
    assert int(d.stats[0, 0]) == 4096 and int(d.stats[0, 1]) == (2 * radius + 1) ** 2


@pytest.mark.parametrize("with_colors", [True, False])
def test_large(built_lib, with_colors):
    """300 000 rows (1 172 blocks), C = 2, 200 x 320, the defaults of render_points"""
    o = large_ref(with_colors)
    d = _run(large_case(with_colors))
    _same_as_ref(d, o, with_colors)
    assert (d.color is None) == (not with_colors) and (o["stats"][:, 1:] > 5000).all()


@pytest.mark.parametrize("with_counts", [True, False])
def test_ragged_batch_equals_single_calls_and_runs_are_identical(built_lib, with_counts):
    """B = 3, valid = (1, 0, 1), the cameras of every problem its own; with counts (1500, 0, 1100) and without any, where `valid`
    alone empties the second problem"""
    from roma_amd import render_points
    cs, refs = ragged_batch(), ragged_refs(with_counts)
    stack = lambda k, dt: _dev(np.stack([c[k] for c in cs]), dt)  # noqa: E731
    args = (stack("points", np.float32), stack("cameras", np.float64), stack("R", np.float64), stack("t", np.float64), cs[0]["H"], cs[0]["W"])
    kw = dict(colors=stack("colors", np.uint8), counts=_dev(RAGGED_COUNTS, np.int32) if with_counts else None, valid=_dev(RAGGED_VALID, np.uint8))
    d, again = render_points(*args, **kw), render_points(*args, **kw)
    assert _equal(d, again)
    for b, c in enumerate(cs):
        one = render_points(*(x[b] if isinstance(x, torch.Tensor) else x for x in args), colors=kw["colors"][b],
                            counts=kw["counts"][b:b + 1] if with_counts else None, valid=kw["valid"][b:b + 1])
        assert _equal([x[b] for x in d], one), b
        _same_as_ref(one, refs[b], b)
    assert not bool(d.stats[1].any()) and bool(torch.isnan(d.depth[1]).all()) and bool((d.index[1] == -1).all()) and not bool(d.mask[1].any())
    assert not bool(d.color[1].any()) and bool((d.stats[0, :, 1] > 500).all()) and bool((d.stats[2, :, 1] > 500).all())


def test_no_rows_render_empty_and_no_problems_launch_nothing(built_lib):
    from roma_amd import render_points
    c = hand_made()
    cam, R, t = (_dev(c[k], np.float64) for k in ("cameras", "R", "t"))
    d = render_points(torch.zeros((0, 3), device=DEV), cam, R, t, 8, 8, colors=torch.zeros((0, 3), device=DEV, dtype=torch.uint8), background=(9, 8, 7))
    _same_as_ref(d, ref(dict(c, points=c["points"][:0], colors=c["colors"][:0], count=None)), "N = 0")
    assert bool(torch.isnan(d.depth).all()) and bool((d.index == -1).all()) and not bool(d.mask.any()) and not bool(d.stats.any())
    assert bool((d.color == torch.tensor([9, 8, 7], device=DEV, dtype=torch.uint8)).all())
    d = render_points(torch.zeros((0, 5, 3), device=DEV), cam, R, t, 8, 8)
    assert d.color is None and tuple(d.depth.shape) == (0, 1, 8, 8) and tuple(d.stats.shape) == (0, 1, 4)


def _guarded(shape, dtype, poison):
    """a tensor inside a poisoned buffer with 256 bytes of guard on both sides"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 512,), 0xA5, device=DEV, dtype=torch.uint8)
    view = buf[256:256 + n].view(dtype).reshape(shape)
    view.fill_(poison)
    return buf, view


def _raw(lib, c, fill, with_colors=True, expect_ok=True, **over):
    """the C entry on guarded outputs and a guarded workspace pre-filled with `fill`; over: arguments replaced to provoke a refusal"""
    kw = dict(dict(radius=1, near=1e-6, far=math.inf, occlusion_radius=2, occlusion_rel=0.05, occlusion_count=3, fill_radius=1, fill_min=3),
              **c["kw"])
    bg = kw.pop("background", (0, 0, 0))
    Cn, H, W, N = len(c["cameras"]), c["H"], c["W"], len(c["points"])
    points, colors = _dev(c["points"], np.float32), (_dev(c["colors"], np.uint8) if with_colors else None)
    cam, R, t = (_dev(c[k], np.float64) for k in ("cameras", "R", "t"))
    count = None if c["count"] is None else _dev([c["count"]], np.int32)
    nws = int(lib.roma_op_render_points_workspace(1, Cn, H, W))
    ws = torch.full((256 + nws + 256,), fill, device=DEV, dtype=torch.uint8)
    ws[:256], ws[256 + nws:] = 0x5A, 0x5A
    outs = [_guarded((Cn, H, W, 3), torch.uint8, 0x77) if with_colors else (None, None), _guarded((Cn, H, W), torch.float32, -7.0),
            _guarded((Cn, H, W), torch.int32, -7), _guarded((Cn, H, W), torch.uint8, 0x77), _guarded((Cn, 4), torch.int32, -7)]
    p = lambda x: C.c_void_p(x.data_ptr() if x is not None else 0)  # noqa: E731
    a = dict(points=p(points), colors=p(colors), counts=p(count), valid=None, cam=p(cam), R=p(R), t=p(t), B=1, N=N, C=Cn, H=H, W=W,
             radius=kw["radius"], near=kw["near"], far=kw["far"], o=kw["occlusion_radius"], rel=kw["occlusion_rel"], oc=kw["occlusion_count"],
             f=kw["fill_radius"], fm=kw["fill_min"], bg=bg[0] | bg[1] << 8 | bg[2] << 16, color=p(outs[0][1]), depth=p(outs[1][1]),
             index=p(outs[2][1]), mask=p(outs[3][1]), stats=p(outs[4][1]), ws=C.c_void_p(ws[256:].data_ptr()), nws=nws)
    a.update(over)
    before = [None if buf is None else buf.clone() for buf, _ in outs]
    torch.cuda.synchronize()
    rc = lib.roma_op_render_points(a["points"], a["colors"], a["counts"], a["valid"], a["cam"], a["R"], a["t"], a["B"], a["N"], a["C"], a["H"], a["W"],
                                   a["radius"], a["near"], a["far"], a["o"], a["rel"], a["oc"], a["f"], a["fm"], a["bg"], a["color"], a["depth"],
                                   a["index"], a["mask"], a["stats"], a["ws"], a["nws"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nws:] == 0x5A).all()), "the band around the workspace"
    if not expect_ok:
        assert rc != 0, over
        for b0, (buf, _) in zip(before, outs):  # refused before anything is enqueued: nothing written
            assert buf is None or bool((buf == b0).all()), over
        assert bool((ws[256:256 + nws] == fill).all()), over
        return lib.roma_last_error().decode()
    assert rc == 0, lib.roma_last_error()
    for k, (buf, _) in zip(KEYS, outs):
        assert buf is None or (bool((buf[:256] == 0xA5).all()) and bool((buf[-256:] == 0xA5).all())), k
    return {k: (None if v is None else v.cpu().numpy()) for k, (_, v) in zip(KEYS, outs)}


def test_workspace_content_does_not_matter_and_nothing_is_written_outside(built_lib):
    c = dict(random_case(), kw=random_kw(1, "o2c3", "f1m3"))
    o = random_ref(1, "o2c3", "f1m3")
    for fill in (0xFF, 0x3C):
        _same_as_ref(_raw(built_lib, c, fill), o, fill)  # every element of every output is written: none keeps its poison
    _same_as_ref(_raw(built_lib, c, 0x00, with_colors=False), dict(o, color=None), "no colours")
    h = hand_made()
    check_hand_made(_raw(built_lib, h, 0x00))


def test_refusals_write_nothing(built_lib):
    c = dict(hand_made(), kw=dict(HAND_KW))
    nan = math.nan
    cases = [(dict(points=None), "null pointer"), (dict(cam=None), "null pointer"), (dict(R=None), "null pointer"), (dict(t=None), "null pointer"),
             (dict(depth=None), "null pointer"), (dict(index=None), "null pointer"), (dict(mask=None), "null pointer"),
             (dict(stats=None), "null pointer"), (dict(colors=None), "go together"), (dict(color=None), "go together"), (dict(C=0), "C >= 1"),
             (dict(B=65536), "65535"), (dict(H=0), "positive"), (dict(W=0), "positive"), (dict(N=-1), "N must"), (dict(radius=5), "[0, 4]"),
             (dict(radius=-1), "[0, 4]"), (dict(o=5), "[0, 4]"), (dict(f=5), "[0, 4]"), (dict(oc=0), "at least 1"), (dict(fm=0), "at least 1"),
             (dict(rel=-0.5), "occlusion_rel"), (dict(rel=nan), "occlusion_rel"), (dict(near=0.0), "near"), (dict(near=nan), "near"),
             (dict(far=0.25), "far"), (dict(far=nan), "far"), (dict(H=26755, W=26755), "2^31"), (dict(nws=16), "workspace too small"),
             (dict(ws=None), "workspace too small")]
    for over, word in cases:
        assert word in _raw(built_lib, c, 0x3C, expect_ok=False, **over), (over, word)
    before = _raw(built_lib, c, 0x3C)
    check_hand_made(before)  # and the entry still works after all of them


def _matcher(weights0, **kw):
    from roma_amd import roma_model
    sd, dsd = weights0
    return roma_model((112, 112), True, device=DEV, weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                      upsample_res=(168, 168), **kw)


def test_chain_renders_the_fused_cloud_back_into_its_views(built_lib, weights0):
    """`fuse_image_set` on the ground-truth warps of four views, as test_gpu_depth_fusion.py runs it; the cloud rendered into each
    source view's own grid camera with radius 0 and both passes off.  Every emitted point with source (v, q) must leave a finite
    depth at pixel q of camera v that is at most fused depth[v, q] (1 + 1e-5).  The margin is derived, not measured: the cloud
    stores fl32(X_w), which moves the depth by at most about 3 * 2^-24 |X_w| / z and the pixel by far less than the half cell to
    the boundary (the point is the centre of its cell); the scene has |X_w| <= 10 z, asserted below, so the depth moves by at
    most about 1.8e-6 - and a pixel holds the nearest of the rows that fall into it."""
    from roma_amd import orbit_cameras
    c = chain_case()
    model = _matcher(weights0, max_batch=1)
    fused = model.fuse_image_set(_dev(c["warp"], np.float32), _dev(c["certainty"], np.float32), c["pairs"], c["K"], _dev(c["R"], np.float64),
                                 _dev(c["t"], np.float64), c["sizes"], min_certainty=0.5)
    H, W, V = c["H"], c["W"], c["V"]
    Kg = np.stack([c["K"][v] * np.array([[W / w], [H / h], [1.0]]) for v, (h, w) in enumerate(CHAIN_SIZES)])
    R, t = _dev(c["R"], np.float64), _dev(c["t"], np.float64)
    back = model.render_fusion(fused, Kg, R, t, H, W, radius=0, occlusion_radius=0, fill_radius=0)
    n = int(fused.counts)
    assert n > 1000 and back.color is None and tuple(back.depth.shape) == (V, H, W)
    src, X = fused.source[:n].cpu().numpy().astype(np.int64), fused.points[:n].cpu().numpy().astype(np.float64)
    zf = fused.depth.cpu().numpy().reshape(V, -1)[src[:, 0], src[:, 1]].astype(np.float64)
    assert np.isfinite(zf).all() and (np.linalg.norm(X, axis=1) <= 10.0 * zf).all()  # what the margin assumes of the case
    zr = back.depth.cpu().numpy().reshape(V, -1)[src[:, 0], src[:, 1]].astype(np.float64)
    print(f"largest rendered / fused depth - 1 over {n} points: {np.nanmax(zr / zf - 1.0):.3e}")
    assert np.isfinite(zr).all() and (zr <= zf * (1.0 + 1e-5)).all()
    # a turntable with the defaults: shapes, dtypes, stats against the masks, rows below counts
    Ro, to = orbit_cameras(c["R"][0], c["t"][0], [0.0, 0.0, 5.0], np.linspace(0.0, 0.6, 5), device=DEV)
    turn = model.render_fusion(fused, Kg[0], Ro, to, H, W)
    assert turn.color is None and turn.depth.dtype == torch.float32 and turn.index.dtype == torch.int32 and turn.mask.dtype == torch.uint8
    assert tuple(turn.depth.shape) == tuple(turn.index.shape) == tuple(turn.mask.shape) == (5, H, W) and tuple(turn.stats.shape) == (5, 4)
    mask, stats, index = turn.mask.cpu().numpy(), turn.stats.cpu().numpy(), turn.index.cpu().numpy()
    for bit in range(3):
        assert np.array_equal(((mask >> bit) & 1).reshape(5, -1).sum(axis=1), stats[:, bit + 1]), bit
    assert (stats[:, 0] <= n).all() and (stats[:, 1] > 200).all() and index.min() >= -1 and index.max() < n
    have = index >= 0
    assert np.array_equal(have, np.isfinite(turn.depth.cpu().numpy())) and np.array_equal(have, (mask & 1).astype(bool) & ~((mask & 2) != 0) | ((mask & 4) != 0))
    own = model.render_fusion(fused, Kg[0], R[:1], t[:1], H, W)
    assert _equal([None if x is None else x[:1] for x in turn], own)  # angle 0 is the view's own camera
    colours = model.render_fusion(fused._replace(colors=torch.full_like(fused.points, 200, dtype=torch.uint8)), Kg[0], Ro, to, H, W, background=(1, 2, 3))
    col = colours.color.cpu().numpy()
    assert col.dtype == np.uint8 and col.shape == (5, H, W, 3) and (col[have] == 200).all() and (col[~have] == (1, 2, 3)).all()
