"""tools/triangulate_ref.py (the oracle of roma_amd.triangulate / triangulate_warp / depth_consistency) against exact geometry, every
flag bit produced on purpose, the scenes tests/test_gpu_triangulate.py runs and the condition that test puts on them (no quantity
within 1e-9 relative of a threshold), and the C ABI of roma_op_triangulate / roma_op_depth_consistency (dlopen only).  No GPU."""
import functools
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import triangulate_ref as tr  # noqa: E402

NEW_SYMBOLS = ("roma_op_triangulate", "roma_op_depth_consistency")
SIZES = (640, 480, 512, 360)  # W_a, H_a, W_b, H_b: two different cameras and image sizes (480 x 640 and 360 x 512)
K_A = np.array([[520.0, 0.0, 325.0], [0.0, 510.0, 236.0], [0.0, 0.0, 1.0]])
K_B = np.array([[430.0, 0.0, 250.0], [0.0, 425.0, 185.0], [0.0, 0.0, 1.0]])
# thresholds of the sparse and the dense GPU tests: every bit of the flag byte occurs under them
THRESHOLDS = dict(max_depth=30.0, max_reproj=1.5, min_parallax=0.5, min_certainty=0.25)
PLANE_H, PLANE_W = 24, 32
DENSE_H, DENSE_W = 23, 31  # row length 62, n = 1426: the half boundary falls inside a wave, the last wave is partial
SPARSE_N, SPARSE_COUNTS = 1003, (1003, 517, 0)
PLANE_SEED, DENSE_SEEDS, SPARSE_SEEDS = 0, (11, 12), (21, 22, 23)


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def project(K, X):
    p = X @ K.T
    return p[..., :2] / p[..., 2:3]


def grid(H, W):
    """normalised pixel centres of an H x W grid, float32 as a matcher stores them: [H, W, 2]"""
    gx = ((np.arange(W) + 0.5) / W * 2.0 - 1.0).astype(np.float32)
    gy = ((np.arange(H) + 0.5) / H * 2.0 - 1.0).astype(np.float32)
    return np.stack(np.meshgrid(gx, gy), axis=-1)


def rays(K, pix):
    return np.stack([(pix[..., 0] - K[0, 2]) / K[0, 0], (pix[..., 1] - K[1, 2]) / K[1, 1], np.ones(pix.shape[:-1])], axis=-1)


@functools.lru_cache(maxsize=None)
def plane_scene(H, W, seed, noise_px=0.0):
    """The tilted plane n . X = 4 (camera A's frame) seen by two different cameras, as a symmetric warp on an H x 2W grid in
    normalised coordinates: the left half holds A's grid and its exact image in B, the right half B's grid and its exact image
    in A (both rounded to float32; Gaussian noise of noise_px pixels on the predicted side).  The truth is computed from the
    float32 grid coordinates, which the triangulation takes as exact.  Returns a dict: warp [H, 2W, 4] float32, R, t, depth_A,
    depth_B [H, W] float64 (the analytic depths)."""
    rng = np.random.default_rng(seed)
    R = rodrigues([0.2 + 0.2 * rng.random(), 1.0, 0.1 * rng.random()], -(0.10 + 0.04 * rng.random()))
    t = np.array([0.50 + 0.1 * rng.random(), 0.04 * rng.random(), 0.10 + 0.05 * rng.random()])
    nrm = np.array([0.15, -0.10, 1.0])
    nrm = nrm / np.linalg.norm(nrm)
    Wa, Ha, Wb, Hb = SIZES
    ga, gb = grid(H, W), grid(H, W)
    xa = rays(K_A, tr.to_pixels(ga, Wa, Ha))
    za = 4.0 / (xa @ nrm)
    pb = project(K_B, (xa * za[..., None]) @ R.T + t)
    nb, cb = R @ nrm, 4.0 + (R @ nrm) @ t  # the plane in camera B's frame: nb . X = cb
    xb = rays(K_B, tr.to_pixels(gb, Wb, Hb))
    zb = cb / (xb @ nb)
    pa = project(K_A, (xb * zb[..., None] - t) @ R)
    if noise_px > 0:
        pb = pb + noise_px * rng.standard_normal(pb.shape)
        pa = pa + noise_px * rng.standard_normal(pa.shape)
    to_norm = lambda p, w, h: np.stack([2.0 * p[..., 0] / w - 1.0, 2.0 * p[..., 1] / h - 1.0], axis=-1).astype(np.float32)  # noqa: E731
    left = np.concatenate([ga, to_norm(pb, Wb, Hb)], axis=-1)
    right = np.concatenate([to_norm(pa, Wa, Ha), gb], axis=-1)
    return {"warp": np.concatenate([left, right], axis=1).astype(np.float32), "R": R, "t": t, "depth_A": za, "depth_B": zb}


@functools.lru_cache(maxsize=None)
def dense_scene(seed):
    """the noisy plane on the DENSE_H x DENSE_W grid with a certainty, a NaN coordinate in each half and a few gross outliers"""
    s = dict(plane_scene(DENSE_H, DENSE_W, seed, noise_px=0.5))
    rng = np.random.default_rng(seed + 1000)
    warp = s["warp"].copy()
    bad = rng.random((DENSE_H, 2 * DENSE_W)) < 0.1
    col = np.arange(2 * DENSE_W)[None, :, None] >= DENSE_W  # right half: the prediction is columns 0:2
    rnd = rng.uniform(-1, 1, (DENSE_H, 2 * DENSE_W, 2)).astype(np.float32)
    warp[..., 0:2] = np.where(bad[..., None] & col, rnd, warp[..., 0:2])
    warp[..., 2:4] = np.where(bad[..., None] & ~col, rnd, warp[..., 2:4])
    warp[3, 5, 2] = np.nan
    warp[7, DENSE_W + 4, 1] = np.nan
    s["warp"] = warp
    s["certainty"] = rng.random((DENSE_H, 2 * DENSE_W)).astype(np.float32)
    return s


@functools.lru_cache(maxsize=None)
def sparse_scene(seed, forward=False):
    """SPARSE_N matches in pixels on a relief (depth 3 .. 5) with 0.5 px noise and 20 % uniform outliers, K_A != K_B, and special
    rows: 0 a point behind both cameras, 1 the image of the ray's point at infinity, 2 a NaN coordinate and - forward (pure
    forward motion, whose epipole is the principal point and so exact in float32) - 3 a reference pixel at the epipole.
    Returns a dict: matches [N, 4] float32, certainty [N] float32, R, t."""
    rng = np.random.default_rng(seed)
    Wa, Ha, Wb, Hb = SIZES
    if forward:
        R, t = np.eye(3), np.array([0.0, 0.0, 0.5])
    else:
        R = rodrigues([0.3 * rng.random(), 1.0, 0.2 * rng.random()], -(0.08 + 0.05 * rng.random()))
        t = np.array([0.5 + 0.1 * rng.random(), 0.05 * rng.random(), 0.1 * rng.random()])
    pa = (rng.random((SPARSE_N, 2)) * [Wa, Ha]).astype(np.float32)
    x = rays(K_A, pa.astype(np.float64))
    z = 4.0 + 0.6 * np.sin(pa[:, 0] / Wa * 5.0 + 1.0) + 0.4 * np.cos(pa[:, 1] / Ha * 4.0 + 2.0)
    z[0] = -3.0
    pb = project(K_B, (x * z[:, None]) @ R.T + t) + 0.5 * rng.standard_normal((SPARSE_N, 2))
    bad = rng.random(SPARSE_N) < 0.2
    pb = np.where(bad[:, None], rng.random((SPARSE_N, 2)) * [Wb, Hb], pb)
    pb[0] = project(K_B, (x[0] * z[0]) @ R.T + t)
    pb[1] = project(K_B, x[1] @ R.T)
    m = np.concatenate([pa, pb.astype(np.float32)], axis=1)
    m[2, 3] = np.nan
    if forward:
        m[3, 0:2] = K_A[0, 2], K_A[1, 2]
    return {"matches": m.astype(np.float32), "certainty": rng.random(SPARSE_N).astype(np.float32), "R": R, "t": t}


def sparse_pairs():
    return [sparse_scene(SPARSE_SEEDS[0]), sparse_scene(SPARSE_SEEDS[1], forward=True), sparse_scene(SPARSE_SEEDS[2])]


def oracle_warp(s, H, W, **kw):
    return tr.triangulate(s["warp"].reshape(-1, 4), s["R"], s["t"], K_A, K_B, coords=1, sizes=SIZES, sym_w=W, **kw)


def scaled_block(points, H, W, scale=1.2, y0=9, x0=14, size=6):
    """[H, 2W, 3] points with one size x size block of the B half scaled away from its camera"""
    p = np.array(points, dtype=np.float32).reshape(H, 2 * W, 3).copy()
    p[y0:y0 + size, W + x0:W + x0 + size] *= np.float32(scale)
    return p


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_reproduces_both_analytic_depths_of_a_plane():
    """z_ref against the analytic depth in both directions.  The bound is the rounding of the predicted coordinate to float32
    (half an ulp, 2^-24 relative, in each normalised coordinate, scaled to pixels) over the disparity - the distance of the
    prediction from the image of the ray's point at infinity -, which is what depth is inversely proportional to; a factor 2
    for the second order.  The reference pixel is taken as exact by the rule, and the truth is computed from it."""
    H, W = PLANE_H, PLANE_W
    s = plane_scene(H, W, PLANE_SEED)
    o = oracle_warp(s, H, W)
    assert np.all(o["flags"] == 0) and not o["near"].any()
    Wa, Ha, Wb, Hb = SIZES
    z = o["points"][:, 2].reshape(H, 2 * W)
    warp = s["warp"].astype(np.float64)
    Ri, ti = tr.inverse_pose(s["R"], s["t"])
    worst = 0.0
    for half, truth, Kr, Ko, Rr, (wr, hr, wo, ho), ref, obs in ((0, s["depth_A"], K_A, K_B, s["R"], (Wa, Ha, Wb, Hb), slice(0, 2), slice(2, 4)),
                                                                (1, s["depth_B"], K_B, K_A, Ri, (Wb, Hb, Wa, Ha), slice(2, 4), slice(0, 2))):
        w = warp[:, half * W:(half + 1) * W]
        p_obs = tr.to_pixels(w[..., obs], wo, ho)
        p_inf = project(Ko, rays(Kr, tr.to_pixels(w[..., ref], wr, hr)) @ Rr.T)
        disparity = np.linalg.norm(p_obs - p_inf, axis=-1)
        delta = 2.0 ** -24 * np.hypot(np.abs(w[..., obs][..., 0]) * wo / 2, np.abs(w[..., obs][..., 1]) * ho / 2)
        rel = np.abs(z[:, half * W:(half + 1) * W] - truth) / truth
        assert np.all(rel <= 2.0 * delta / disparity + 1e-12), (half, rel.max())
        worst = max(worst, rel.max())
    print(f"plane: worst relative depth error of the oracle {worst:.3e}")
    stats = o["stats"]
    assert stats[0, 0] == stats[0, 1] == H * W and stats[1, 0] == stats[1, 1] == H * W
    # other-camera depth of an A point is the depth of the same 3-D point in B
    X = o["points"].reshape(H, 2 * W, 3)[:, :W]
    assert np.allclose((X @ s["R"].T + s["t"])[..., 2], o["depth_other"].reshape(H, 2 * W)[:, :W], rtol=1e-12)
    assert np.abs(o["reproj"]).max() < 1e-4  # exact matches lie on their epipolar lines


def test_consistency_rule_on_the_plane():
    H, W = PLANE_H, PLANE_W
    s = plane_scene(H, W, PLANE_SEED)
    o = oracle_warp(s, H, W)
    cons, err, near = tr.depth_consistency(o["points"].astype(np.float32), o["flags"], s["R"], s["t"], K_A, K_B, SIZES, H, W)
    share = float((cons != 2).mean())
    print(f"plane: supported share {share:.3f}, worst consistency error {np.nanmax(err):.3e}")
    assert 0.8 <= share <= 0.95, share
    assert np.all(cons[cons != 2] == 1) and not near.any()
    assert np.all(np.isnan(err) == (cons == 2))
    # one block of the B half scaled by 1.2: the zeros are the block itself and the A points whose neighbours touch it
    y0, x0, size = 9, 14, 6
    p = scaled_block(o["points"], H, W, 1.2, y0, x0, size)
    cons2, err2, near2 = tr.depth_consistency(p, o["flags"], s["R"], s["t"], K_A, K_B, SIZES, H, W)
    assert not near2.any()
    zero = cons2 == 0
    assert zero[:, :W].any() and zero[:, W:].any()
    inside_block = np.zeros((H, 2 * W), dtype=bool)
    inside_block[y0:y0 + size, W + x0:W + x0 + size] = True
    assert not (zero[:, W:] & ~inside_block[:, W:]).any()
    # an A point is touched if one of its four neighbours lies in the block
    X = o["points"].reshape(H, 2 * W, 3)[:, :W]
    g = project(K_B, X @ s["R"].T + s["t"]) / [SIZES[2], SIZES[3]] * [W, H] - 0.5
    gx0, gy0 = np.floor(g[..., 0]), np.floor(g[..., 1])
    touched = (gx0 + 1 >= x0) & (gx0 <= x0 + size - 1) & (gy0 + 1 >= y0) & (gy0 <= y0 + size - 1)
    assert not (zero[:, :W] & ~touched).any()
    same =np.concatenate([~touched, ~inside_block[:, W:]], axis=1)
    assert np.array_equal(cons2[same], cons[same])
    # an invalid neighbour takes the support away; an invalid point is 2 itself
    f = o["flags"].reshape(H, 2 * W).copy()
    f[12, W + 16] = tr.CHEIRALITY
    cons3, _, _ = tr.depth_consistency(o["points"].astype(np.float32), f, s["R"], s["t"], K_A, K_B, SIZES, H, W)
    assert cons3[12, W + 16] == 2 and (cons3[:, :W] == 2).sum() > (cons[:, :W] == 2).sum()


def test_each_flag_bit_on_purpose():
    R, t = rodrigues([0.1, 1.0, 0.0], -0.1), np.array([0.5, 0.02, 0.05])
    x = np.array([0.1, -0.05, 1.0])
    pa = project(K_A, x)

    def one(pb, pa=pa, R=R, t=t, cert=None, **kw):
        o = tr.triangulate(np.concatenate([pa, pb])[None], R, t, K_A, K_B, certainty=cert, **kw)
        return int(o["flags"][0]), o

    front = project(K_B, R @ (4.0 * x) + t)
    f, o = one(front)
    assert f == 0 and abs(o["points"][0, 2] - 4.0) < 1e-9 and np.allclose(o["points"][0], 4.0 * x, atol=1e-9)
    assert abs(o["depth_other"][0] - (R @ (4.0 * x) + t)[2]) < 1e-9 and abs(o["reproj"][0]) < 1e-9
    Y = R @ (4.0 * x) + t
    want = np.degrees(np.arccos((R @ x) @ Y / np.linalg.norm(R @ x) / np.linalg.norm(Y)))
    assert abs(o["parallax"][0] - want) < 1e-6
    f, o = one(project(K_B, R @ (-3.0 * x) + t))  # behind the camera
    assert f == tr.CHEIRALITY and abs(o["points"][0, 2] + 3.0) < 1e-9
    # the exact image of the point at infinity: with R = I and equal cameras the prediction is the reference pixel, a = 0, w = 0
    pix = np.array([400.0, 300.0])
    o = tr.triangulate(np.concatenate([pix, pix])[None], np.eye(3), np.array([0.5, 0.0, 0.0]), K_A, K_A)
    assert int(o["flags"][0]) == tr.CHEIRALITY and np.isnan(o["points"][0, 2]) and o["parallax"][0] == 0.0
    # a reference pixel at the epipole: forward motion, the principal point
    o = tr.triangulate(np.array([[K_A[0, 2], K_A[1, 2], 200.0, 100.0]]), np.eye(3), np.array([0.0, 0.0, 0.5]), K_A, K_B)
    assert int(o["flags"][0]) == tr.DEGENERATE and np.all(np.isnan(o["points"][0])) and np.isnan(o["reproj"][0])
    f, o = one(front, t=np.zeros(3))  # t = 0: no epipolar line
    assert f == tr.DEGENERATE
    f, o = one(np.array([np.nan, 10.0]))
    assert f == tr.DEGENERATE and np.all(np.isnan(o["points"][0])) and np.isnan(o["parallax"][0])
    Rn = R.copy()
    Rn[1, 1] = np.inf
    assert one(front, R=Rn)[0] == tr.DEGENERATE
    # a row beyond counts, a pair that is not valid
    two = np.stack([np.concatenate([pa, front])] * 2)
    o = tr.triangulate(two, R, t, K_A, K_B, count=1)
    assert list(o["flags"]) == [0, tr.SKIPPED] and np.all(np.isnan(o["points"][1])) and list(o["stats"][0, :2]) == [1, 1]
    o = tr.triangulate(two, R, t, K_A, K_B, valid=False)
    assert list(o["flags"]) == [tr.SKIPPED] * 2 and not o["stats"].any()
    # each of the four thresholds, alone and together
    assert one(front, max_depth=3.9)[0] == tr.CHEIRALITY and one(front, max_depth=4.2)[0] == 0
    off = front + 2.0 * np.array([0.0, 1.0])
    d = abs(one(off)[1]["reproj"][0])
    assert 1.5 < d <= 2.0 and one(off, max_reproj=d * 1.01)[0] == 0 and one(off, max_reproj=d * 0.99)[0] == tr.REPROJ
    assert one(front, min_parallax=want * 1.01)[0] == tr.PARALLAX and one(front, min_parallax=want * 0.99)[0] == 0
    c = np.array([0.5], dtype=np.float32)
    assert one(front, cert=c, min_certainty=0.6)[0] == tr.CERTAINTY and one(front, cert=c, min_certainty=0.5)[0] == 0
    assert one(front, cert=np.array([np.nan], dtype=np.float32))[0] == tr.CERTAINTY
    f, o = one(off, cert=c, max_depth=3.9, max_reproj=1.0, min_parallax=90.0, min_certainty=0.6)
    assert f == tr.CHEIRALITY | tr.REPROJ | tr.PARALLAX | tr.CERTAINTY and list(o["stats"][0]) == [1, 0, 0, 1, 1, 1, 1, 0]
    assert np.isfinite(o["points"][0]).all()  # rows without bit 1 or 2 keep their computed values
    # threshold edges are reported
    assert one(off, max_reproj=d * (1 + 5e-10))[1]["near"][0] and not one(off, max_reproj=d * (1 + 1e-8))[1]["near"][0]


def test_b_reference_is_the_a_reference_rule_with_the_roles_swapped():
    s = dense_scene(DENSE_SEEDS[0])
    H, W = DENSE_H, DENSE_W
    o = oracle_warp(s, H, W, certainty=s["certainty"].reshape(-1), **THRESHOLDS)
    right = s["warp"][:, W:].reshape(-1, 4)
    Ri, ti = tr.inverse_pose(s["R"], s["t"])
    sw = tr.triangulate(right[:, [2, 3, 0, 1]], Ri, ti, K_B, K_A, certainty=s["certainty"][:, W:].reshape(-1), coords=1,
                        sizes=(SIZES[2], SIZES[3], SIZES[0], SIZES[1]), **THRESHOLDS)
    for k in ("points", "depth_other", "reproj", "parallax", "flags"):
        assert np.array_equal(o[k].reshape((H, 2 * W) + o[k].shape[1:])[:, W:].reshape(sw[k].shape), sw[k], equal_nan=k != "flags"), k
    assert np.array_equal(o["stats"][1], sw["stats"][0])


def test_gpu_scenes_have_no_threshold_edges_and_show_every_bit():
    """what tests/test_gpu_triangulate.py relies on, checked here first: no quantity within 1e-9 relative of a threshold it is
    tested against (such a row could fall either way on the device), and the scenes set every bit"""
    bits = 0
    for b, s in enumerate(sparse_pairs()):
        o = tr.triangulate(s["matches"], s["R"], s["t"], K_A, K_B, certainty=s["certainty"], count=SPARSE_COUNTS[b], **THRESHOLDS)
        assert not o["near"].any(), b
        assert not tr.triangulate(s["matches"], s["R"], s["t"], K_A, K_B, certainty=s["certainty"], **THRESHOLDS)["near"].any(), b
        assert np.array_equal(o["stats"][0, 1:7], [(o["flags"] == 0).sum()] + [((o["flags"] & k) != 0).sum() for k in (2, 4, 8, 16, 32)])
        assert o["stats"][0, 0] == SPARSE_COUNTS[b] and not o["stats"][1].any()
        if SPARSE_COUNTS[b]:
            assert o["flags"][0] & tr.CHEIRALITY and o["flags"][1] & tr.CHEIRALITY and o["flags"][2] == tr.DEGENERATE
            assert 0.3 < (o["flags"][:SPARSE_COUNTS[b]] == 0).mean() < 0.8
        if b == 1:
            assert o["flags"][3] == tr.DEGENERATE
        bits |= int(np.bitwise_or.reduce(o["flags"]))
    assert bits == 63
    for seed in DENSE_SEEDS:
        s = dense_scene(seed)
        o = oracle_warp(s, DENSE_H, DENSE_W, certainty=s["certainty"].reshape(-1), **THRESHOLDS)
        assert not o["near"].any() and int(np.bitwise_or.reduce(o["flags"])) == 62 and (o["flags"] == 0).mean() > 0.3
        assert o["stats"][0, 0] == o["stats"][1, 0] == DENSE_H * DENSE_W and o["stats"][0, 2] == o["stats"][1, 2] == 1
    s = plane_scene(PLANE_H, PLANE_W, PLANE_SEED)
    o = oracle_warp(s, PLANE_H, PLANE_W)
    for p in (o["points"].astype(np.float32), scaled_block(o["points"], PLANE_H, PLANE_W)):
        assert not tr.depth_consistency(p, o["flags"], s["R"], s["t"], K_A, K_B, SIZES, PLANE_H, PLANE_W)[2].any()


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert len(_lib.SIGNATURES["roma_op_triangulate"][1]) == 27
    assert len(_lib.SIGNATURES["roma_op_depth_consistency"][1]) == 17


def test_arguments_are_validated_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null 16-byte aligned address: validation must fail before it is used
    inf = float("inf")

    def tri(*, m=p, R=p, t=p, pts=p, fl=p, B=2, n=1000, coords=0, sizes=(0, 0, 0, 0), sym_w=0, th=(inf, inf, 0.0, 0.0)):
        return lib.roma_op_triangulate(m, None, None, None, R, t, None, None, B, n, coords, *sizes, sym_w, *th, pts, None, None, None,
                                       fl, None, None)
    for kw, word in ((dict(m=None), b"null"), (dict(R=None), b"null"), (dict(t=None), b"null"), (dict(pts=None), b"null"),
                     (dict(fl=None), b"null"), (dict(B=-1), b"B"), (dict(B=65536), b"B"), (dict(n=-3), b"negative"),
                     (dict(B=2, n=1 << 30), b"2^31"), (dict(B=3, n=715827883), b"2^31"), (dict(m=8), b"aligned"),
                     (dict(sym_w=7), b"sym_w"), (dict(sym_w=-2), b"sym_w"), (dict(sym_w=1000), b"sym_w"),
                     (dict(coords=1, sizes=(640, 480, 512, 0)), b"sizes"), (dict(coords=1, sizes=(-640, 480, 512, 360)), b"sizes"),
                     (dict(coords=2), b"coords"), (dict(th=(-1.0, inf, 0.0, 0.0)), b"negative"), (dict(th=(inf, -1.0, 0.0, 0.0)), b"negative"),
                     (dict(th=(inf, inf, -0.5, 0.0)), b"negative"), (dict(th=(inf, inf, 0.0, -0.1)), b"negative")):
        assert tri(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    for kw in (dict(B=0), dict(n=0), dict(B=0, n=0)):
        assert tri(**kw) == 0  # nothing to do, nothing launched

    def cons(*, pts=p, fl=p, R=p, t=p, out=p, sizes=SIZES, B=2, H=24, W=32, rel=0.05):
        return lib.roma_op_depth_consistency(pts, fl, R, t, None, None, *sizes, B, H, W, rel, out, None, None)
    for kw, word in ((dict(pts=None), b"null"), (dict(fl=None), b"null"), (dict(R=None), b"null"), (dict(t=None), b"null"),
                     (dict(out=None), b"null"), (dict(B=-1), b"B"), (dict(B=65536), b"B"), (dict(H=-1), b"negative"),
                     (dict(W=-1), b"negative"), (dict(H=1 << 15, W=1 << 15), b"2^31"), (dict(sizes=(640, 480, 0, 360)), b"sizes"),
                     (dict(rel=-0.1), b"negative")):
        assert cons(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert cons(**kw) == 0


def test_python_front_end_refuses_host_tensors():
    import roma_amd
    from roma_amd import _lib
    from roma_amd.matcher import RegressionMatcher
    for name in ("triangulate", "triangulate_warp", "depth_consistency"):
        assert name in roma_amd.__all__ and callable(getattr(roma_amd, name))
    assert callable(RegressionMatcher.triangulate_warp)
    R, t, K = torch.eye(3, dtype=torch.float64)[None], torch.ones(1, 3, dtype=torch.float64), np.eye(3)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.triangulate(torch.zeros(1, 10, 2), torch.zeros(1, 10, 2), R, t, K, K)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.triangulate(torch.zeros(1, 10, 4), None, R, t, K, K)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.triangulate_warp(torch.zeros(1, 4, 8, 4), torch.zeros(1, 4, 8), R, t, K, K, 480, 640)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.depth_consistency(torch.zeros(1, 4, 8, 3), torch.zeros(1, 4, 8, dtype=torch.uint8), R, t, K, K, 480, 640)
    m = RegressionMatcher.__new__(RegressionMatcher)
    m.symmetric = True
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        m.triangulate_warp(torch.zeros(1, 4, 8, 4), None, R, t, K, K, 480, 640)


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_triangulate_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "triangulate.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/triangulate.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["depth_consistency_kernel", "triangulate_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
