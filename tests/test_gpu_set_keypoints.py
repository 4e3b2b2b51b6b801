"""Device detector-free keypoints (roma_amd.keypoints_from_matches; csrc/set_keypoints.hip) against the numpy restatement
tools/set_keypoints_ref.py: every comparison exact, bit for bit on the floats; then the chain on a scene - keypoints, tracks,
reconstruct_views - against the chain of numpy restatements, and RegressionMatcher.reconstruct_image_set against its manual
composition."""
import ctypes as C

import numpy as np
import pytest
import torch

from set_keypoints_cases import (NORM_THR, RANDOM_PARAMS, THR, chain_for, check_hand_made, hand_made, large_case, ragged_batch, random_case, ref,
                                 scene_case, scene_pose_errors, scene_tracks)
from views_cases import chain_errors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("kpts", "score", "num_kpts", "total", "inds", "kept", "info")


def _dev(x, dtype):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _bits(x):
    x = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _run(c, **kw):
    from roma_amd import keypoints_from_matches
    return keypoints_from_matches(_dev(c["matches"], np.float32), _dev(c["certainty"], np.float32), c["pairs"], c["V"], c["sizes"],
                                  counts=_dev(c["counts"], np.int32), **kw)


def _as_dict(d):
    return {k: v.cpu().numpy() for k, v in zip(KEYS, d)}


def _same_as_ref(d, o, where=""):
    """every output equals the restatement's: the floats bit for bit (the NaN padding compared as NaN)"""
    d = _as_dict(d) if not isinstance(d, dict) else d
    for k in KEYS:
        a, b = np.asarray(d[k]), np.asarray(o[k])
        if k == "kpts":
            assert np.array_equal(np.isnan(a), np.isnan(b)), (where, k)
            a, b = np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0)
        assert a.shape == b.shape and np.array_equal(_bits(a.astype(b.dtype) if a.dtype.kind == "i" else a), _bits(b)), (where, k)


def _pads(d, c):
    """the documented values beyond the counts: kpts NaN and score 0 at and beyond num_kpts, inds -1 at and beyond counts"""
    d = _as_dict(d) if not isinstance(d, dict) else d
    for v, n in enumerate(d["num_kpts"]):
        assert np.isnan(d["kpts"][v, n:]).all() and np.isfinite(d["kpts"][v, :n]).all() and not d["score"][v, n:].any() and (d["score"][v, :n] > 0).all()
    for p, n in enumerate(c["counts"]):
        assert (d["inds"][p, n:] == -1).all()
    assert d["kept"].sum() == d["info"][4] == (d["inds"][..., 0] >= 0).sum()


@pytest.mark.parametrize("radius", [2.0, 0.0])
def test_hand_made(built_lib, radius):
    c = hand_made()
    d = _run(c, cell=2, radius=radius, max_kpts=8)
    check_hand_made(_as_dict(d), radius)
    _same_as_ref(d, ref(c, cell=2, radius=radius, max_kpts=8))


@pytest.mark.parametrize("cell,radius,K,o2o", RANDOM_PARAMS)
def test_random_against_the_restatement(built_lib, cell, radius, K, o2o):
    c = random_case(0)
    kw = dict(cell=cell, radius=radius, max_kpts=K, one_to_one=bool(o2o))
    o = ref(c, **kw)
    d = _run(c, **kw)
    _same_as_ref(d, o, kw)
    _pads(d, c)
    # suppression happens wherever it is on, and max_kpts = 100 cuts (but at cell 3 / radius 3, where no view keeps 100: 93 at most)
    assert o["info"][4] > 0 and (o["info"][5] > 0) == (radius > 0) and (o["total"] > K).any() == (K == 100 and (cell, radius) != (3, 3.0))


def test_large_grid_scan_crosses_many_workgroups(built_lib):
    c = large_case()
    kw = dict(cell=1, max_kpts=65536)
    o = ref(c, **kw)
    d = _run(c, **kw)
    _same_as_ref(d, o)
    H, W = c["sizes"][0]
    for v in range(3):  # kept keypoints in the first and in the last cell of the grid
        n = int(o["num_kpts"][v])
        assert n > 9000 and np.floor(o["kpts"][v, 0]).tolist() == [0, 0] and np.floor(o["kpts"][v, n - 1]).tolist() == [W - 1, H - 1]


def test_ragged_batch_equals_single_calls_and_runs_are_identical(built_lib):
    from roma_amd import keypoints_from_matches
    cs = ragged_batch()
    args = (_dev(np.stack([c["matches"] for c in cs]), np.float32), _dev(np.stack([c["certainty"] for c in cs]), np.float32), cs[0]["pairs"], 4,
            cs[0]["sizes"])
    kw = dict(counts=_dev(np.stack([c["counts"] for c in cs]), np.int32), cell=2, max_kpts=80)
    d = keypoints_from_matches(*args, **kw)
    again = keypoints_from_matches(*args, **kw)
    for x, y in zip(d, again):
        assert np.array_equal(_bits(x), _bits(y))
    for b, c in enumerate(cs):
        one = _run(c, cell=2, max_kpts=80)
        for k, x, y in zip(KEYS, d, one):
            assert np.array_equal(_bits(x[b]), _bits(y)), (b, k)
        _same_as_ref(one, ref(c, cell=2, max_kpts=80), b)
    assert d.info[2].cpu().tolist() == [3600, 3600, 0, 0, 0, 0] and int(d.total[2].sum()) == 0 and bool((d.inds[2] == -1).all())
    assert int(d.total[0].max()) > 80  # the batch takes the cut too


def _guarded(shape, dtype, poison):
    """a tensor inside a poisoned buffer with 256 bytes of guard on both sides"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 512,), 0xA5, device=DEV, dtype=torch.uint8)
    view = buf[256:256 + n].view(dtype).reshape(shape)
    view.fill_(poison)
    return buf, view


def _guards_intact(buf):
    return bool((buf[:256] == 0xA5).all()) and bool((buf[-256:] == 0xA5).all())


def _raw(lib, c, fill, cell=2, radius=2.0, K=100, o2o=1):
    """the C entry on guarded outputs and a guarded workspace pre-filled with `fill`"""
    P, N = c["certainty"].shape
    V = c["V"]
    m, cert, counts = _dev(c["matches"], np.float32), _dev(c["certainty"], np.float32), _dev(c["counts"], np.int32)
    pv = np.ascontiguousarray(np.asarray(c["pairs"], np.int32))
    sz = np.ascontiguousarray(np.asarray(c["sizes"], np.int32))
    g_total = sum(((h + cell - 1) // cell) * ((w + cell - 1) // cell) for h, w in c["sizes"])
    nws = int(lib.roma_op_keypoints_from_matches_workspace(1, V, P, N, g_total, K))
    ws = torch.full((256 + nws + 256,), fill, device=DEV, dtype=torch.uint8)
    ws[:256], ws[256 + nws:] = 0x5A, 0x5A
    outs = [_guarded((V, K, 2), torch.float32, -7.0), _guarded((V, K), torch.float32, -7.0), _guarded((V,), torch.int32, -7),
            _guarded((V,), torch.int32, -7), _guarded((P, N, 2), torch.int32, -7), _guarded((P,), torch.int32, -7), _guarded((6,), torch.int32, -7)]
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = lib.roma_op_keypoints_from_matches(p(m), p(cert), p(counts), pv.ctypes.data, sz.ctypes.data, 1, V, P, N, cell, radius, K, o2o,
                                            *(p(v) for _, v in outs), C.c_void_p(ws[256:].data_ptr()), nws,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, lib.roma_last_error()
    assert bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nws:] == 0x5A).all()), "the band around the workspace"
    for k, (buf, _) in zip(KEYS, outs):
        assert _guards_intact(buf), k
    return {k: v.cpu().numpy() for k, (_, v) in zip(KEYS, outs)}


def test_workspace_content_does_not_matter_and_nothing_is_written_outside(built_lib):
    c = random_case(0)
    o = ref(c, cell=2, radius=2.0, max_kpts=100)
    a = _raw(built_lib, c, 0xFF)
    b = _raw(built_lib, c, 0x00)
    for d in (a, b):
        _same_as_ref(d, o)  # every element of every output is written: none keeps its poison
        _pads(d, c)
    off = _raw(built_lib, c, 0xFF, radius=0.0, K=4096, o2o=0)
    _same_as_ref(off, ref(c, cell=2, radius=0.0, max_kpts=4096, one_to_one=False))


def _scene_device(radius):
    from roma_amd import build_tracks
    case, scene = scene_case()
    d = _run(case, cell=2, radius=radius)
    tr = build_tracks(d.inds, case["pairs"], case["V"], match_counts=_dev(case["counts"], np.int32), num_kpts=d.num_kpts, kpts=d.kpts)
    return case, scene, d, tr


def test_chain_on_a_scene(built_lib):
    """views_scene(5, False) shifted to start at 0, every pair's endpoints jittered by +-0.25 px on their own, cell 2: the device
    equals the restatement bit for bit, so the gates of test_cpu_set_keypoints.py hold for both - tracks 290 of the 292 points
    seen in two views or more (99.3 %; gate >= 90 %), 1 component dropped (0.3 %; gate <= 5 %), 173 tracks (59.2 %; gate < 75 %)
    with radius 0.  reconstruct_views on the device tracks is held to twice the pose errors of the chain of numpy restatements on
    the same tracks, with the exact-data figures of views_cases.ref_chain as the floor.  Measured on an MI355X: device rotation
    1.044e-2 deg, translation direction 8.142e-2 deg; the numpy chain on the same tracks 1.044e-2 / 8.142e-2 (the device takes the
    chain's RANSAC samples); floor 1.2e-6 / 4.8e-6."""
    from roma_amd import reconstruct_views
    case, scene, d, tr = _scene_device(None)
    o = ref(case, cell=2)
    _same_as_ref(d, o)
    t_ref = scene_tracks(o, case)
    n = scene["seen2"]
    total, info = int(tr.total), tr.info.cpu().tolist()
    assert total == t_ref["total"] and info == list(t_ref["info"])
    assert np.array_equal(tr.kpts[:, :total].cpu().numpy(), t_ref["kpts"][:, :total], equal_nan=True)
    _, _, d0, tr0 = _scene_device(0.0)
    print(f"{n} points in two views or more: tracks {total} ({total / n:.1%}), components dropped {info[3]} ({info[3] / n:.1%}); "
          f"radius 0: tracks {int(tr0.total)} ({int(tr0.total) / n:.1%})")
    assert total >= 0.9 * n and info[3] <= 0.05 * n and int(tr0.total) < 0.75 * n and int(d0.info[5]) == 0 and int(d.info[5]) > 0
    r = reconstruct_views(tr.kpts, scene["K"], NORM_THR, THR, counts=tr.counts, seed=3)
    assert bool(r.ok) and bool(r.view_ok.all())
    er, et = scene_pose_errors(scene, r.R.cpu().numpy(), r.t.cpu().numpy(), np.ones(4, bool))
    chain = chain_for(t_ref["kpts"][:, :total], scene["K"])
    cr, ct = scene_pose_errors(scene, chain["R"], chain["t"], chain["view_ok"])
    fr, ft = chain_errors(5, False)
    print(f"device: rotation {er:.3e} deg, translation direction {et:.3e} deg; numpy chain on the same tracks: {cr:.3e}, {ct:.3e}; "
          f"exact-data floor {fr:.3e}, {ft:.3e}")
    assert chain["view_ok"].all() and er <= max(2 * cr, fr) and et <= max(2 * ct, ft)


def test_no_host_synchronisation(built_lib):
    from roma_amd import build_tracks, keypoints_from_matches, reconstruct_views
    case, scene = scene_case()
    m, c, n = _dev(case["matches"], np.float32), _dev(case["certainty"], np.float32), _dev(case["counts"], np.int32)
    Kd, seed = _dev(scene["K"], np.float64), torch.tensor([3]).to(DEV)

    def chain():
        d = keypoints_from_matches(m, c, case["pairs"], 4, case["sizes"], counts=n, cell=2)
        tr = build_tracks(d.inds, case["pairs"], 4, match_counts=n, num_kpts=d.num_kpts, kpts=d.kpts)
        return d, tr, reconstruct_views(tr.kpts, Kd, NORM_THR, THR, counts=tr.counts, seed=seed)

    first = chain()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = chain()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)


def test_reconstruct_image_set_is_its_manual_composition(built_lib, weights0):
    """Synthetic weights, three small images, coarse resolution 112.  The warps of random weights carry no geometry, so this
    checks only the plumbing: it runs, the shapes are right, it equals the manual composition bit for bit, and 9 images are
    refused."""
    from roma_amd import build_tracks, reconstruct_views, roma_model
    sd, dsd = weights0
    model = roma_model((112, 112), True, device=DEV, weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                       upsample_res=(168, 168), max_batch=3)
    g = np.random.default_rng(5)
    sizes = [(120, 160), (96, 128), (150, 110)]
    ims = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    K = np.array([[[200.0, 0, w / 2], [0, 200.0, h / 2], [0, 0, 1]] for h, w in sizes])
    rec, tr, kp = model.reconstruct_image_set(ims, K, NORM_THR, THR, num=500, seed=7, max_kpts=1024)
    assert tuple(kp.kpts.shape) == (3, 1024, 2) and tuple(kp.inds.shape) == (3, 500, 2) and tuple(kp.info.shape) == (6,)
    assert tuple(tr.kpts.shape) == (3, 1024, 2) and tuple(rec.R.shape) == (3, 3, 3) and tuple(rec.points.shape) == (1024, 3)
    nk = kp.num_kpts.cpu().numpy()
    for v, (h, w) in enumerate(sizes):  # the keypoints lie inside their own image
        x = kp.kpts[v, :nk[v]].cpu().numpy()
        assert nk[v] > 0 and (x >= 0).all() and (x[:, 0] < w).all() and (x[:, 1] < h).all()
    warp, cert, pairs = model.match_image_set(ims)
    kp2, counts = model.set_keypoints(warp, cert, pairs, sizes, num=500, seed=7, max_kpts=1024)
    tr2 = build_tracks(kp2.inds, pairs, 3, match_counts=counts, num_kpts=kp2.num_kpts, kpts=kp2.kpts)
    rec2 = reconstruct_views(tr2.kpts, K, NORM_THR, THR, counts=tr2.counts, seed=7)
    for a, b in zip((rec, tr, kp), (rec2, tr2, kp2)):
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="2 .. 8"):
        model.reconstruct_image_set([ims[0]] * 9, K, NORM_THR, THR)
