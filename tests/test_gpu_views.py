"""Device track building, N-view triangulation and reconstruct_views (roma_amd.build_tracks / triangulate_views /
reconstruct_views; csrc/tracks.hip, csrc/triangulate_views.hip) against their numpy restatements tools/tracks_ref.py and
tools/triangulate_views_ref.py: everything exact for the tracks, flags / used / stats exact and points within LM_TOL for the
triangulation, and the chain of restatements for reconstruct_views."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from views_cases import (HAND_MADE_INFO, HAND_MADE_TRACKS, NORM_THR, SHAPES, THR, chain_errors, f32, hand_made, planted, pose_errors, ref_chain,
                         scene, track_ref, tri_case, tvr, views_scene, zigzag)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# largest entry of |X| device - oracle: the bound the sibling fits are held to (test_gpu_bundle.LM_TOL, ten times the 7.2e-10
# measured for refine_pose) on scenes of size 4; every test that uses it prints its figure
LM_TOL = 7.2e-9


def _dev(x, dtype=np.float64):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _bits(x):
    x = x.cpu().numpy()
    return x.view(np.int32) if x.dtype == np.float32 else x.view(np.int64) if x.dtype == np.float64 else x


def _equal(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- build_tracks
def _tracks(c, **kw):
    from roma_amd import build_tracks
    return build_tracks(_dev(c["inds"], np.int32), [tuple(p) for p in c["pairs"]], c["V"], match_counts=_dev(c["match_counts"], np.int32),
                        num_kpts=None if c["num_kpts"] is None else _dev(c["num_kpts"], np.int32), kpts=_dev(c["x"], np.float32), **kw)


def _check_tracks(c, d, **kw):
    o = track_ref(c, **kw)
    assert d.index.dtype == torch.int32 and d.kpts.dtype == torch.float32 and tuple(d.index.shape) == o["tracks"].shape
    assert np.array_equal(d.index.cpu().numpy(), o["tracks"]) and int(d.counts) == o["count"] and int(d.total) == o["total"]
    assert tuple(d.info.cpu().tolist()) == o["info"], (d.info.cpu().tolist(), o["info"])
    assert np.array_equal(d.kpts.cpu().numpy().view(np.int32), o["kpts"].view(np.int32))  # the keypoint's bits, one NaN elsewhere
    return o


def test_build_tracks_hand_made(built_lib):
    c = hand_made()
    d = _tracks(c)
    o = _check_tracks(c, d)
    assert o["total"] == 2 and np.array_equal(d.index.cpu().numpy()[:, :2], HAND_MADE_TRACKS) and tuple(d.info.cpu().tolist()) == HAND_MADE_INFO
    assert _equal(d, _tracks(c))
    # without the keypoints only the indices come back
    from roma_amd import build_tracks
    e = build_tracks(_dev(c["inds"], np.int32), [tuple(p) for p in c["pairs"]], 3, match_counts=_dev(c["match_counts"], np.int32),
                     num_kpts=_dev(c["num_kpts"], np.int32), kpts_per_view=5)
    assert e.kpts is None and torch.equal(e.index, d.index) and torch.equal(e.info, d.info)


@pytest.mark.parametrize("permute", [False, True])
def test_build_tracks_zigzag_path(built_lib, permute):
    c = zigzag(permute)
    o = _check_tracks(c, _tracks(c))
    assert o["total"] == 10 and o["info"] == (2059, 0, 11, 1)


def test_build_tracks_eight_views_all_pairs(built_lib):
    c = planted(8, 257, 0)
    d = _tracks(c)
    o = _check_tracks(c, d)
    lengths = (o["tracks"][:, :o["total"]] >= 0).sum(axis=0)
    print(f"{o['total']} tracks, lengths {np.bincount(lengths)[2:].tolist()}, info {o['info']}")
    assert set(lengths.tolist()) == set(range(2, 9)) and o["info"][3] > 0
    assert _equal(d, _tracks(c))
    _check_tracks(c, _tracks(c, min_views=3), min_views=3)
    # T smaller than the total: the first T tracks, and total tells the rest
    T = o["total"] // 2
    few = _tracks(c, max_tracks=T)
    _check_tracks(c, few, max_tracks=T)
    assert int(few.counts) == T and int(few.total) == o["total"] and torch.equal(few.index, d.index[:, :T])


def test_build_tracks_at_eight_views_of_16384_keypoints(built_lib):
    """8 x 16 384 nodes - the labels no longer fit a workgroup's LDS - with tracks spread over the whole index range"""
    c = planted(8, 16384, 4, n_tracks=1500)
    o = _check_tracks(c, _tracks(c, max_tracks=2048), max_tracks=2048)
    print(f"{o['total']} tracks, info {o['info']}")
    assert o["total"] > 1000 and o["tracks"].max() > 16000


def test_build_tracks_ragged_batch_equals_single_calls(built_lib):
    from roma_amd import build_tracks
    cases = [planted(4, 300, 1, num_kpts=[300, 257, 129, 64]), planted(4, 300, 2, num_kpts=[1, 300, 300, 300], false_frac=0.2), planted(4, 300, 3, n_tracks=0)]
    M = max(c["inds"].shape[1] for c in cases)
    inds = np.full((3, 6, M, 2), 7, dtype=np.int32)  # rows beyond match_counts would join keypoints 7
    for b, c in enumerate(cases):
        inds[b, :, :c["inds"].shape[1]] = c["inds"]
    pairs = [tuple(p) for p in cases[0]["pairs"]]
    args = dict(match_counts=_dev(np.stack([c["match_counts"] for c in cases]), np.int32),
                num_kpts=_dev(np.stack([c["num_kpts"] if c["num_kpts"] is not None else np.full(4, 300) for c in cases]), np.int32),
                kpts=_dev(np.stack([c["x"] for c in cases]), np.float32))
    inds = _dev(inds, np.int32)
    d = build_tracks(inds, pairs, 4, **args)
    assert tuple(d.index.shape) == (3, 4, 300) and d.total.cpu().tolist()[2] == 0 and d.total.cpu().tolist()[0] > 0
    for b, c in enumerate(cases):
        one = _tracks(c)
        _check_tracks(c, one)
        assert _equal([o[b] for o in d], one), b
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = build_tracks(inds, pairs, 4, **args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _equal(d, again)


GUARD = 8


def _guarded(shape, dtype, poison):
    """(buffer, the output inside it): GUARD rows of poison, at least 16 elements, in front of the output and behind it"""
    n, pad = int(np.prod(shape)), 16 * (-(-GUARD * int(shape[-1]) // 16))  # a multiple of 16 elements keeps the output aligned
    buf = torch.full((pad + n + pad,), poison, device=DEV, dtype=dtype)
    return buf, buf[pad:pad + n].view(*shape)


def _guards_intact(buf, v, poison):
    pad = (buf.numel() - v.numel()) // 2
    return bool((buf[:pad] == poison).all()) and bool((buf[pad + v.numel():] == poison).all())


def test_build_tracks_guard_bytes_and_a_poisoned_workspace(built_lib):
    lib = built_lib
    c = planted(8, 257, 0)
    B, V, K, T = 2, 8, 257, 100
    P, M = c["inds"].shape[:2]
    inds, x = _dev(np.stack([c["inds"]] * B), np.int32), _dev(np.stack([c["x"]] * B), np.float32)
    mc = _dev(np.stack([c["match_counts"]] * B), np.int32)
    outs = [_guarded((B, V, T), torch.int32, -7), _guarded((B, V, T, 2), torch.float32, -7.0), _guarded((B,), torch.int32, -7),
            _guarded((B,), torch.int32, -7), _guarded((B, 4), torch.int32, -7)]
    nws = int(lib.roma_op_build_tracks_workspace(B, V, K, P, M))
    wsbuf = torch.full((256 + nws + 256,), 0xFF, device=DEV, dtype=torch.uint8)
    ws = wsbuf[256:256 + nws]
    pv = np.ascontiguousarray(c["pairs"], dtype=np.int32)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = lib.roma_op_build_tracks(p(inds), pv.ctypes.data, p(mc), None, p(x), B, V, K, P, M, T, 2, *(p(v) for _, v in outs), p(ws), nws,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    o = track_ref(c, max_tracks=T)
    for b in range(B):
        assert np.array_equal(outs[0][1][b].cpu().numpy(), o["tracks"]) and np.array_equal(outs[1][1][b].cpu().numpy().view(np.int32), o["kpts"].view(np.int32))
        assert int(outs[2][1][b]) == T and int(outs[3][1][b]) == o["total"] and tuple(outs[4][1][b].cpu().tolist()) == o["info"]
    for buf, v in outs:
        assert _guards_intact(buf, v, -7)  # nothing written in front of the output or behind it
    assert bool((wsbuf[:256] == 0xFF).all()) and bool((wsbuf[256 + nws:] == 0xFF).all())


# ---- triangulate_views
def _triangulate(s, **kw):
    from roma_amd import triangulate_views
    return triangulate_views(_dev(s["kpts"], np.float32), s["K"], _dev(s["R"]), _dev(s["t"]), **kw)


@pytest.mark.parametrize("trim", [False, True], ids=["all", "trim"])
@pytest.mark.parametrize("noisy", [False, True], ids=["exact", "noisy"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_triangulate_views_against_oracle(built_lib, name, noisy, trim):
    s, o, left_out = tri_case(name, noisy, trim)
    d = _triangulate(s, max_reproj=THR if noisy else math.inf, trim=trim)
    assert d.points.dtype == torch.float64 and d.reproj.dtype == torch.float32 and d.used.dtype == torch.bool and d.flags.dtype == torch.uint8
    assert tuple(d.points.shape) == (len(left_out), 3) and tuple(d.reproj.shape) == s["kpts"].shape[:2] and tuple(d.stats.shape) == (8,)
    assert left_out.sum() <= 0.01 * len(left_out)
    keep = ~left_out
    flags, used, pts = d.flags.cpu().numpy(), d.used.cpu().numpy(), d.points.cpu().numpy()
    assert np.array_equal(flags[keep], o["flags"][keep]) and np.array_equal(used[:, keep], o["used"][:, keep])
    assert np.array_equal(d.valid.cpu().numpy(), flags == 0)
    if not left_out.any():
        assert tuple(d.stats.cpu().tolist()) == o["stats"], (d.stats.cpu().tolist(), o["stats"])
    has = keep & ((o["flags"] & 3) == 0)
    diff = np.abs(pts - o["points"])[has].max()
    rdiff = np.nanmax(np.abs(d.reproj.cpu().numpy() - o["reproj"])[:, has])
    pdiff = np.abs(d.parallax.cpu().numpy() - o["parallax"])[has].max()
    print(f"{name}: stats {o['stats']}, |dX| {diff:.3e}, |d reproj| {rdiff:.3e} px, |d parallax| {pdiff:.3e} deg, {left_out.sum()} points left out")
    assert diff <= LM_TOL, diff
    assert np.isnan(pts[keep & ~has]).all() and np.isnan(d.parallax.cpu().numpy()[keep & ~has]).all()
    assert np.array_equal(np.isnan(d.reproj.cpu().numpy())[:, keep], np.isnan(o["reproj"])[:, keep])
    assert rdiff <= 1e-3 and pdiff <= 1e-4  # f32 outputs of f64 values that agree to LM_TOL: pixels of a 640 image, degrees


def test_triangulate_views_view_valid_counts_and_batch(built_lib):
    from roma_amd import triangulate_views
    s, o, _ = tri_case("v8", True, True)
    kp = _dev(s["kpts"], np.float32)
    vv = torch.tensor([1, 1, 0, 1, 1, 0, 1, 1], device=DEV, dtype=torch.bool)
    a = _triangulate(s, max_reproj=THR, view_valid=vv)
    k2 = kp.clone()
    k2[~vv] = float("nan")
    b = triangulate_views(k2, s["K"], _dev(s["R"]), _dev(s["t"]), max_reproj=THR)
    assert _equal(a, b) and int(a.stats[1]) > 0 and not bool(a.used[~vv].any())
    # a pose that is not finite takes its view out, and nothing else
    R2 = _dev(s["R"]).clone()
    R2[2, 0, 0], R2[5, 1, 1] = float("nan"), float("inf")
    assert _equal(a, triangulate_views(kp, s["K"], R2, _dev(s["t"]), max_reproj=THR))
    # B = 3 with counts and valid: skipped rows carry flag 1 and NaN; every problem is its own B = 1 call
    s3, _, _ = tri_case("v3", True, True)
    N = 513
    kb = _dev(np.stack([s3["kpts"]] * 3), np.float32)
    kb[1] = kb[1].flip(1)
    Rb, tb = _dev(np.stack([s3["R"]] * 3)), _dev(np.stack([s3["t"]] * 3))
    counts, valid = torch.tensor([513, 257, 400]), torch.tensor([True, True, False])
    run = lambda: triangulate_views(kb, s3["K"], Rb, tb, counts=counts, valid=valid, max_reproj=THR)  # noqa: E731
    d = run()
    assert _equal(d, run())
    f = d.flags.cpu().numpy()
    assert (f[1, 257:] == tvr.SKIPPED).all() and (f[2] == tvr.SKIPPED).all() and not (f[0] & 1).any() and not (f[1, :257] & 1).any()
    assert bool(torch.isnan(d.points[1, 257:]).all()) and bool(torch.isnan(d.points[2]).all()) and not bool(d.used[2].any())
    assert bool(torch.isnan(d.reproj[1, :, 257:]).all()) and d.stats[:, 0].cpu().tolist() == [513, 257, 0] and d.stats[2].cpu().tolist() == [0] * 8
    for i, c in ((0, 513), (1, 257)):
        one = triangulate_views(kb[i, :, :c], s3["K"], Rb[i], tb[i], max_reproj=THR)
        assert _equal([d.points[i, :c], d.reproj[i, :, :c], d.used[i, :, :c], d.parallax[i, :c], d.flags[i, :c], d.stats[i]],
                      [one.points, one.reproj, one.used, one.parallax, one.flags, one.stats]), i
    Kd, cd, vd = _dev(s3["K"]), counts.to(DEV), valid.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = triangulate_views(kb, Kd, Rb, tb, counts=cd, valid=vd, max_reproj=THR)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _equal(d, again)


def test_triangulate_views_parallel_rays_and_thresholds(built_lib):
    from roma_amd import triangulate_views
    s = scene(3, 12, 4)
    kp = f32(s["kpts"])
    kp[1, 0] = kp[0, 0]  # two identical rays from two views with the same pose
    R, t, K = s["R"].copy(), s["t"].copy(), s["K"].copy()
    R[1], t[1], K[1] = R[0], t[0], K[0]
    kp[2, 0], kp[1, 1:] = np.nan, np.nan
    o = tvr.triangulate(kp, K, R, t)
    d = triangulate_views(_dev(kp, np.float32), K, _dev(R), _dev(t))
    f = d.flags.cpu().numpy()
    assert f[0] == tvr.DEGENERATE and np.array_equal(f, o["flags"]) and bool(torch.isnan(d.points[0]).all()) and not bool(d.used[:, 0].any())
    assert bool(torch.isfinite(d.points[1:]).all()) and np.abs(d.points.cpu().numpy() - o["points"])[1:].max() <= LM_TOL
    assert tuple(d.stats.cpu().tolist()) == o["stats"]
    # depth and parallax thresholds, min_views, no refinement steps
    s8, _, _ = tri_case("v8", False, False)
    for kw in (dict(max_depth=4.0, min_parallax=5.0), dict(min_views=4), dict(gn_steps=0), dict(gn_steps=10, max_reproj=0.5)):
        o = tvr.triangulate(s8["kpts"], s8["K"], s8["R"], s8["t"], **kw)
        d = _triangulate(s8, **kw)
        has = (o["flags"] & 3) == 0
        assert np.array_equal(d.flags.cpu().numpy(), o["flags"]) and tuple(d.stats.cpu().tolist()) == o["stats"], kw
        assert np.abs(d.points.cpu().numpy() - o["points"])[has].max() <= LM_TOL and has.sum() > 0, kw


def test_triangulate_views_guard_bytes(built_lib):
    lib = built_lib
    s, o, _ = tri_case("v8", True, True)
    B, V, N = 1, 8, 130
    kp, K, R, t = _dev(s["kpts"][None], np.float32), _dev(s["K"][None]), _dev(s["R"][None]), _dev(s["t"][None])
    outs = [_guarded((B, N, 3), torch.float64, -7.0), _guarded((B, V, N), torch.float32, -7.0), _guarded((B, V, N), torch.uint8, 77),
            _guarded((B, N), torch.float32, -7.0), _guarded((B, N), torch.uint8, 77), _guarded((B, 8), torch.int32, -7)]
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = lib.roma_op_triangulate_views(p(kp), p(K), p(R), p(t), None, None, None, B, V, N, THR, 0.0, math.inf, 2, 3, 1, *(p(v) for _, v in outs),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(outs[4][1][0].cpu().numpy(), o["flags"]) and tuple(outs[5][1][0].cpu().tolist()) == o["stats"]
    for (buf, v), poison in zip(outs, (-7.0, -7.0, 77, -7.0, 77, -7)):
        assert _guards_intact(buf, v, poison)


# ---- reconstruct_views
def _reconstruct(s, **kw):
    from roma_amd import reconstruct_views
    return reconstruct_views(_dev(s["kpts"], np.float32), s["K"], NORM_THR, THR, seed=3, **kw)


def _bound(noisy, seed=5, rng_seed=3):
    """twice the pose errors of the chain of numpy restatements on the same scene, with the exact-data figure as the floor"""
    er, et = chain_errors(seed, noisy, rng_seed=rng_seed)
    fr, ft = chain_errors(5, False)
    return max(2 * er, fr), max(2 * et, ft)


def _check_reconstruction(s, r, noisy, views=(0, 1, 2, 3), seed=5, rng_seed=3):
    R, t, X = r.R.cpu().numpy(), r.t.cpu().numpy(), r.points.cpu().numpy()
    ok = np.array([v in views for v in range(4)])
    assert bool(r.ok) and r.view_ok.cpu().tolist() == ok.tolist()
    cost = r.cost.cpu().numpy()
    assert cost[1] <= cost[0]
    assert np.array_equal(R[0], np.eye(3)) and not t[0].any()
    er, et = pose_errors(dict(R=s["R"][ok], t=s["t"][ok]), R[ok], t[ok])
    br_, bt_ = _bound(noisy, seed, rng_seed)
    print(f"rotation {er:.3e} deg (bound {br_:.3e}), translation direction {et:.3e} deg (bound {bt_:.3e}), cost {cost[0]:.3e} -> {cost[1]:.3e}")
    assert er <= br_ and et <= bt_
    return R, t, X


@pytest.mark.parametrize("noisy", [False, True], ids=["exact", "noisy"])
def test_reconstruct_views_against_the_reference_chain(built_lib, noisy):
    s = views_scene(5, noisy)
    r = _reconstruct(s)
    R, t, X = _check_reconstruction(s, r, noisy)
    assert r.points.dtype == torch.float64 and tuple(r.mask.shape) == (4, 300) and tuple(r.t.shape) == (4, 3) and tuple(r.info.shape) == (6,)
    # NaN exactly where a track has fewer than two observations in registered views or was flagged: the points' start is the
    # triangulation from the poses the registration gave, which bundle_adjust moves but never adds to or takes from
    seen = np.isfinite(s["kpts"]).all(axis=2).sum(axis=0)
    assert np.isnan(X[seen < 2]).all() and np.isfinite(X).all(axis=1).sum() > (150 if noisy else 250)
    assert not bool(r.mask[:, torch.as_tensor(np.isnan(X).any(axis=1), device=DEV)].any())
    if not noisy:
        assert np.array_equal(np.isnan(X).any(axis=1), seen < 2)
    # and where the chain of restatements, which takes the same samples, has none
    assert np.array_equal(np.isnan(X).any(axis=1), np.isnan(ref_chain(5, noisy)["points"]).any(axis=1))


def test_reconstruct_views_batch_dead_view_and_no_synchronisation(built_lib):
    from roma_amd import reconstruct_views
    a, b = views_scene(5, True), views_scene(6, True)
    kp = _dev(np.stack([a["kpts"], b["kpts"]]), np.float32)
    seeds = torch.tensor([3, 4])
    out = reconstruct_views(kp, a["K"], NORM_THR, THR, seed=seeds)
    assert tuple(out.R.shape) == (2, 4, 3, 3) and tuple(out.points.shape) == (2, 300, 3) and bool(out.ok.all()) and bool(out.view_ok.all())
    one = _reconstruct(a)
    assert _equal([o[0] for o in out], one)
    for i, (s, sc, sd) in enumerate(((a, 5, 3), (b, 6, 4))):
        print(f"problem {i}:")
        _check_reconstruction(s, type(out)(*(o[i] for o in out)), True, seed=sc, rng_seed=sd)
    # view 3 without an observation: not registered, identity and held, the others as before within the same bound
    dead = views_scene(5, True, dead_view=3)
    r = _reconstruct(dead)
    R, t, X = _check_reconstruction(a, r, True, views=(0, 1, 2))
    assert np.array_equal(R[3], np.eye(3)) and not t[3].any() and not bool(r.mask[3].any())
    Kd, sd = _dev(a["K"]), seeds.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = reconstruct_views(kp, Kd, NORM_THR, THR, seed=sd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _equal(out, again)
