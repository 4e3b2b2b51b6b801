"""roma_amd.triangulate / triangulate_warp / depth_consistency (roma_op_triangulate, roma_op_depth_consistency) against
tools/triangulate_ref.py on the scenes of tests/test_cpu_triangulate.py, which also asserts that none of them holds a quantity
within 1e-9 relative of a threshold.

Float bound (derived, not tuned): both sides run the same float64 operations in the same order with correctly rounded
+ - * / sqrt; they differ only in atan2's last bits and in the final rounding to float32.  So points, depth_other, parallax and err
must lie within 2 float32 ulps of the oracle's value, reproj within 2 ulps + 1e-9 px."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulate_ref as tr  # noqa: E402
import test_cpu_triangulate as S  # noqa: E402  (the scenes)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOATS = ("points", "depth_other", "reproj", "parallax")


def _dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _np(x):
    return x.detach().cpu().numpy()


def assert_floats_match(name, got, want, extra=0.0):
    """|got - want| <= 2 float32 ulps of want (+ extra); the same NaN and infinities.  Returns the worst difference in ulps."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float64)
    with np.errstate(over="ignore"):
        w32 = want.astype(np.float32)
    fin = np.isfinite(w32)
    assert np.array_equal(np.isnan(got), np.isnan(w32)), name
    assert np.array_equal(got[~fin & ~np.isnan(w32)], w32[~fin & ~np.isnan(w32)]), name
    ulp = np.spacing(np.abs(w32[fin])).astype(np.float64)
    diff = np.abs(got[fin].astype(np.float64) - want[fin])
    worst = float((np.maximum(diff - extra, 0.0) / ulp).max()) if fin.any() else 0.0
    print(f"{name}: worst difference {worst:.3f} float32 ulps ({float(diff.max()) if fin.any() else 0.0:.3e})")
    assert worst <= 2.0, (name, worst)
    return worst


def compare(tag, got, want):
    """a device Triangulation (one pair) against the oracle's dict"""
    assert not want["near"].any(), tag
    assert np.array_equal(_np(got.flags), want["flags"]), tag
    assert np.array_equal(_np(got.valid), want["flags"] == 0), tag
    assert np.array_equal(_np(got.stats), want["stats"]), (tag, _np(got.stats), want["stats"])
    for k in FLOATS:
        assert_floats_match(f"{tag} {k}", _np(getattr(got, k)), want[k], 1e-9 if k == "reproj" else 0.0)


def sparse_batch():
    pairs = S.sparse_pairs()
    m = _dev(np.stack([p["matches"] for p in pairs]))
    c = _dev(np.stack([p["certainty"] for p in pairs]))
    R, t = _dev(np.stack([p["R"] for p in pairs])), _dev(np.stack([p["t"] for p in pairs]))
    return pairs, m, c, R, t


def warp_batch(scenes):
    w = _dev(np.stack([s["warp"] for s in scenes]))
    R, t = _dev(np.stack([s["R"] for s in scenes])), _dev(np.stack([s["t"] for s in scenes]))
    return w, R, t


def test_sparse_matches_the_oracle(built_lib):
    """item 1: B = 3, N = 1003, counts (1003, 517, 0), pixels, K_A != K_B, noise, outliers and the special rows"""
    import roma_amd
    pairs, m, c, R, t = sparse_batch()
    counts = torch.tensor(S.SPARSE_COUNTS, device=DEV, dtype=torch.int32)
    out = roma_amd.triangulate(m[..., :2], m[..., 2:], R, t, S.K_A, S.K_B, certainty=c, counts=counts, **S.THRESHOLDS)
    assert tuple(out.points.shape) == (3, S.SPARSE_N, 3) and out.flags.dtype == torch.uint8 and out.valid.dtype == torch.bool
    flags = _np(out.flags)
    for b, p in enumerate(pairs):
        want = tr.triangulate(p["matches"], p["R"], p["t"], S.K_A, S.K_B, certainty=p["certainty"], count=S.SPARSE_COUNTS[b],
                              **S.THRESHOLDS)
        compare(f"sparse pair {b}", roma_amd.triangulation.Triangulation(*(o[b] for o in out)), want)
        f = flags[b]
        pop = [(f != tr.SKIPPED).sum(), (f == 0).sum()] + [((f & k) != 0).sum() for k in (2, 4, 8, 16, 32)] + [0]
        assert np.array_equal(_np(out.stats)[b, 0], pop) and not _np(out.stats)[b, 1].any()
    # the [B, N, 4] form reads the tensor in place and gives the same bits; so does the single-pair form
    out4 = roma_amd.triangulate(m, None, R, t, S.K_A, S.K_B, certainty=c, counts=counts, **S.THRESHOLDS)
    one = roma_amd.triangulate(m[0], None, R[0], t[0, :, None], _dev(S.K_A), _dev(S.K_B), certainty=c[0], **S.THRESHOLDS)
    for a, b4, o1 in zip(out, out4, one):
        assert torch.equal(a, b4) or torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b4, nan=-7.0))
        assert tuple(o1.shape) == tuple(a.shape[1:])
        assert torch.equal(torch.nan_to_num(a[0].float(), nan=-7.0), torch.nan_to_num(o1.float(), nan=-7.0))


def test_dense_symmetric_matches_the_oracle(built_lib):
    """item 2: B = 2, H = 23, W = 31 (row length 62, n = 1426), normalised coordinates, different image sizes; the right half is
    bit-equal to a second call on the swapped columns with the inverse pose passed in"""
    import roma_amd
    scenes = [S.dense_scene(seed) for seed in S.DENSE_SEEDS]
    H, W = S.DENSE_H, S.DENSE_W
    w, R, t = warp_batch(scenes)
    c = _dev(np.stack([s["certainty"] for s in scenes]))
    Wa, Ha, Wb, Hb = S.SIZES
    out = roma_amd.triangulate_warp(w, c, R, t, S.K_A, S.K_B, Ha, Wa, Hb, Wb, symmetric=True, **S.THRESHOLDS)
    assert tuple(out.depth_A.shape) == (2, H, W) and tuple(out.points_B.shape) == (2, H, W, 3) and out.valid_B.dtype == torch.bool
    for b, s in enumerate(scenes):
        want = S.oracle_warp(s, H, W, certainty=s["certainty"].reshape(-1), **S.THRESHOLDS)
        assert not want["near"].any()
        assert np.array_equal(_np(out.stats[b]), want["stats"])
        for half, name in enumerate("AB"):
            sel = lambda x: x.reshape((H, 2 * W) + x.shape[1:])[:, half * W:(half + 1) * W]  # noqa: E731
            assert np.array_equal(_np(out[f"flags_{name}"][b]), sel(want["flags"]))
            assert np.array_equal(_np(out[f"valid_{name}"][b]), sel(want["flags"]) == 0)
            assert_floats_match(f"dense {b} points_{name}", _np(out[f"points_{name}"][b]), sel(want["points"]))
            assert_floats_match(f"dense {b} reproj_{name}", _np(out[f"reproj_{name}"][b]), sel(want["reproj"]), 1e-9)
            assert_floats_match(f"dense {b} parallax_{name}", _np(out[f"parallax_{name}"][b]), sel(want["parallax"]))
            assert torch.equal(torch.nan_to_num(out[f"depth_{name}"][b], nan=-7.0), torch.nan_to_num(out[f"points_{name}"][b, ..., 2], nan=-7.0))
    # the B half alone, as A-reference points of the swapped problem: the inverse pose comes from the oracle's restatement of
    # the kernel's own (R^T, -R^T t)
    inv = [tr.inverse_pose(s["R"], s["t"]) for s in scenes]
    Ri, ti = _dev(np.stack([i[0] for i in inv])), _dev(np.stack([i[1] for i in inv]))
    right = w[:, :, W:][..., [2, 3, 0, 1]].contiguous()
    sw = roma_amd.triangulate_warp(right, c[:, :, W:].contiguous(), Ri, ti, S.K_B, S.K_A, Hb, Wb, Ha, Wa, symmetric=False, **S.THRESHOLDS)
    for k in ("points", "depth", "reproj", "parallax", "flags", "valid"):
        a, b = out[f"{k}_B"], sw[f"{k}_A"]
        assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0)), k
    assert torch.equal(out.stats[:, 1], sw.stats[:, 0])


def test_exact_geometry(built_lib):
    """item 3: on the plane the device's depth error against the truth is at most the oracle's plus the float bound"""
    import roma_amd
    H, W = S.PLANE_H, S.PLANE_W
    s = S.plane_scene(H, W, S.PLANE_SEED)
    w, R, t = warp_batch([s])
    Wa, Ha, Wb, Hb = S.SIZES
    out = roma_amd.triangulate_warp(w[0], None, R[0], t[0], S.K_A, S.K_B, Ha, Wa, Hb, Wb, symmetric=True)
    assert tuple(out.depth_A.shape) == (H, W) and bool(out.valid_A.all()) and bool(out.valid_B.all())
    want = S.oracle_warp(s, H, W)["points"][:, 2].reshape(H, 2 * W)
    for half, name in enumerate("AB"):
        truth = s[f"depth_{name}"]
        z = _np(out[f"depth_{name}"]).astype(np.float64)
        e_dev, e_ref = np.abs(z - truth), np.abs(want[:, half * W:(half + 1) * W] - truth)
        print(f"plane depth_{name}: device error {np.max(e_dev / truth):.3e} relative, oracle {np.max(e_ref / truth):.3e}")
        assert np.all(e_dev <= e_ref + 2.0 * np.spacing(truth.astype(np.float32)).astype(np.float64))


def test_determinism_batch_independence_and_pair_order(built_lib):
    """item 4"""
    import roma_amd
    scenes = [S.dense_scene(S.DENSE_SEEDS[0]), S.dense_scene(S.DENSE_SEEDS[1]), dict(S.plane_scene(S.DENSE_H, S.DENSE_W, 5, 0.3))]
    scenes[2]["certainty"] = scenes[0]["certainty"][::-1].copy()
    w, R, t = warp_batch(scenes)
    c = _dev(np.stack([s["certainty"] for s in scenes]))
    Wa, Ha, Wb, Hb = S.SIZES
    KA, KB = _dev(S.K_A), _dev(S.K_B)

    def run(idx):
        o = roma_amd.triangulate_warp(w[idx], c[idx], R[idx], t[idx], KA, KB, Ha, Wa, Hb, Wb, symmetric=True, consistency=True,
                                      **S.THRESHOLDS)
        return {k: torch.nan_to_num(v.float(), nan=-7.0) for k, v in o.items()}
    first, again, one, perm = run([0, 1, 2]), run([0, 1, 2]), run([1]), run([2, 0, 1])
    for k in first:
        assert torch.equal(first[k], again[k]), k
        assert torch.equal(first[k][1:2], one[k]), k
        assert torch.equal(first[k][[2, 0, 1]], perm[k]), k
    assert int((first["consistent_A"] == 1).sum()) > 0


def test_skipped_pairs(built_lib):
    """item 5: valid = (1, 0, 1) leaves the middle pair's flags at 1, its floats NaN and its stats rows zero"""
    import roma_amd
    pairs, m, c, R, t = sparse_batch()
    R[1] = float("nan")  # a pair that is not valid is never read
    valid = torch.tensor([True, False, True], device=DEV)
    out = roma_amd.triangulate(m, None, R, t, S.K_A, S.K_B, certainty=c, valid=valid, **S.THRESHOLDS)
    assert bool((out.flags[1] == tr.SKIPPED).all()) and not bool(out.valid[1].any()) and not bool(out.stats[1].any())
    for k in FLOATS:
        assert bool(torch.isnan(getattr(out, k)[1]).all()), k
    for b in (0, 2):
        want = tr.triangulate(pairs[b]["matches"], pairs[b]["R"], pairs[b]["t"], S.K_A, S.K_B, certainty=pairs[b]["certainty"], **S.THRESHOLDS)
        compare(f"valid pair {b}", roma_amd.triangulation.Triangulation(*(o[b] for o in out)), want)


def test_consistency_matches_the_oracle(built_lib):
    """item 6: the plane with one 6 x 6 block of the B half scaled by 1.2 after triangulation"""
    import roma_amd
    H, W = S.PLANE_H, S.PLANE_W
    s = S.plane_scene(H, W, S.PLANE_SEED)
    w, R, t = warp_batch([s])
    Wa, Ha, Wb, Hb = S.SIZES
    out = roma_amd.triangulate_warp(w, None, R, t, S.K_A, S.K_B, Ha, Wa, Hb, Wb, symmetric=True, consistency=True)
    points = torch.cat((out.points_A, out.points_B), dim=2)
    flags = torch.cat((out.flags_A, out.flags_B), dim=2)
    cons0 = np.concatenate([_np(out.consistent_A[0]), _np(out.consistent_B[0])], axis=1)
    want0, err0, near0 = tr.depth_consistency(_np(points[0]), _np(flags[0]), s["R"], s["t"], S.K_A, S.K_B, S.SIZES, H, W)
    assert not near0.any() and np.array_equal(cons0, want0) and not (cons0 == 0).any() and 0.8 <= (cons0 != 2).mean() <= 0.95
    moved = S.scaled_block(_np(points[0]), H, W)
    cons, err = roma_amd.depth_consistency(_dev(moved)[None], flags, R, t, S.K_A, S.K_B, Ha, Wa, Hb, Wb, return_err=True)
    want, werr, near = tr.depth_consistency(moved, _np(flags[0]), s["R"], s["t"], S.K_A, S.K_B, S.SIZES, H, W)
    assert not near.any() and np.array_equal(_np(cons[0]), want)
    assert_floats_match("consistency err", _np(err[0]), werr)
    zero = want == 0
    assert zero[:, :W].any() and zero[:, W:].any() and not zero[:, W:][:9].any() and not zero[:, W:][:, :14].any()
    assert np.array_equal(want[~zero], want0[~zero])  # the block's footprint is the only change
    single = roma_amd.depth_consistency(_dev(moved), flags[0], R[0], t[0], S.K_A, S.K_B, Ha, Wa, Hb, Wb)
    assert torch.equal(single, cons[0])


def test_cheirality_agrees_with_recover_pose(built_lib):
    """item 7: exact correspondences, some in front and some behind: flags & 4 == 0 is recover_pose's mask_good for the same
    (R, t) with max_depth = distance_thresh.  Noisy rows are left out on purpose: the two triangulations differ off the line."""
    import roma_amd
    rng = np.random.default_rng(31)
    R = S.rodrigues([0.2, 1.0, -0.1], 0.12)
    t = np.array([0.8, 0.1, -0.2])
    t = t / np.linalg.norm(t)
    n = 600
    x = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), np.ones((n, 1))], axis=1)
    z = rng.uniform(2.0, 80.0, n)
    z[400:] *= -1.0  # behind
    Y = (x * z[:, None]) @ R.T + t
    xa, xb = x[:, :2].astype(np.float32), (Y[:, :2] / Y[:, 2:3]).astype(np.float32)
    E = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]]) @ R
    dist = 50.0
    a, b = _dev(xa)[None], _dev(xb)[None]
    n_good, Rd, td, good = roma_amd.recover_pose(_dev(E)[None], a, b, distance_thresh=dist)
    out = roma_amd.triangulate(a, b, Rd, td, None, None, max_depth=dist)
    want = tr.triangulate(np.concatenate([xa, xb], axis=1), _np(Rd[0]), _np(td[0]), max_depth=dist)
    assert not want["near"].any()
    front = (out.flags & tr.CHEIRALITY) == 0
    assert torch.equal(front, good) and int(n_good[0]) == int(front.sum())
    assert 200 < int(front.sum()) < 400  # in front and nearer than dist in both cameras
    assert np.allclose(_np(Rd[0]), R, atol=1e-5) and np.allclose(_np(td[0]).reshape(3), t, atol=1e-5)


def test_chain_runs_without_synchronisation(built_lib):
    """item 8: sample_matches -> estimate_pose(counts=...) -> triangulate_warp with no host synchronisation; the result is the
    oracle's for the device's pose; the median relative depth error against the truth, scaled by |t_true|, is printed"""
    import accuracy_harness as AH
    import roma_amd
    h, w = 48, 64
    pair = AH.synthetic_relief_pair(h, w, seed=3)
    warp = pair["gt_matches"].to(DEV)[None].repeat(2, 1, 1, 1).contiguous()
    cert = pair["gt_certainty"].to(DEV)[None].repeat(2, 1, 1).contiguous()
    K = torch.as_tensor(pair["K1"], device=DEV)
    seeds = torch.tensor([4, 5], device=DEV)
    thr = 0.5 / float(pair["K1"][0, 0])

    def chain():
        m, c, counts = roma_amd.sample_matches(warp, cert, num=1000, seed=seeds, return_counts=True)
        ka = torch.stack(((m[..., 0] + 1) * (w / 2), (m[..., 1] + 1) * (h / 2)), dim=-1)
        kb = torch.stack(((m[..., 2] + 1) * (w / 2), (m[..., 3] + 1) * (h / 2)), dim=-1)
        R, t, mask, ok = roma_amd.estimate_pose(ka, kb, K, K, thr, seed=seeds, counts=counts)
        return R, t, ok, roma_amd.triangulate_warp(warp, cert, R, t, K, K, h, w, symmetric=False, valid=ok, min_certainty=0.5)
    chain()  # warm-up: library, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        R, t, ok, out = chain()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(ok.all()) and tuple(out.depth_A.shape) == (2, h, w) and "depth_B" not in out
    T = pair["T_1to2"]
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    gen = torch.Generator().manual_seed(3)  # the harness's relief, from its own first two random numbers
    r1, r2 = torch.rand(1, generator=gen).item(), torch.rand(1, generator=gen).item()
    truth = 4.0 + 0.6 * np.sin(xs / w * 5.0 + 6.0 * r1) + 0.4 * np.cos(ys / h * 4.0 + 6.0 * r2)
    for b in range(2):
        want = tr.triangulate(_np(warp[b]).reshape(-1, 4), _np(R[b]), _np(t[b]), pair["K1"], pair["K2"],
                              certainty=_np(cert[b]).reshape(-1), coords=1, sizes=(w, h, w, h), min_certainty=0.5)
        assert not want["near"].any()
        assert np.array_equal(_np(out.flags_A[b]).reshape(-1), want["flags"]) and np.array_equal(_np(out.stats[b]), want["stats"])
        assert_floats_match(f"chain {b} points", _np(out.points_A[b]).reshape(-1, 3), want["points"])
        v = _np(out.valid_A[b])
        z = _np(out.depth_A[b]).astype(np.float64) * np.linalg.norm(T[:, 3])  # the estimated t has unit length
        rel = np.abs(z[v] - truth[v]) / truth[v]
        print(f"chain pair {b}: {int(v.sum())} valid points, median relative depth error {np.median(rel):.3e}")
        assert v.any() and np.isfinite(rel).all()
