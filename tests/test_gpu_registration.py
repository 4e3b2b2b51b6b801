"""Device registration (roma_amd.align_points / similarity_minimal / refine_similarity / fit_similarity / apply_similarity /
depth_rows / register_depth_maps / trajectory_error, csrc/registration.hip) against its numpy restatement
tools/registration_ref.py and against exact geometry; tails, ragged counts, determinism, the far origin, and the chain of two
reconstructions joined by one similarity.  Everything the device is compared with goes through f32 first: the oracle gets what
the device sees."""
import math

import numpy as np
import pytest
import torch

from registration_cases import (AGREEMENT, RAGGED_COUNTS, REFINE_SEEDS, agreement_scene, collinear_samples, depth_case, exact_samples, f32,
                                model_error, ragged_batch, random_samples, residual, rr, scene, trajectory_case, umeyama_svd)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# |R_device - R_oracle|_F, |t_device - t_oracle| and |s_device - s_oracle| of the refinement: the bound test_gpu_absolute_pose.py
# and test_gpu_pose_refine.py hold their fits to
LM_TOL = 7.2e-9


def _dev(x, dtype=np.float32):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


def _np(x):
    return x.cpu().numpy()


def _start(model):
    return tuple(_dev(v, np.float64) for v in model)


def test_minimal_solver_matches_the_oracle(built_lib):
    from roma_amd import similarity_minimal
    Xe, Ye, st, Rt, tt = exact_samples(4096, seed=3)
    Xr, Yr = random_samples(4096, seed=4)
    Xc, Yc = collinear_samples(64, seed=5)
    X, Y = np.concatenate([Xe, Xr, Xc]), np.concatenate([Ye, Yr, Yc])
    for with_scale in (True, False):
        s, R, t, n = similarity_minimal(_dev(X, np.float64), _dev(Y, np.float64), with_scale)
        assert tuple(R.shape) == (8256, 3, 3) and tuple(t.shape) == (8256, 3) and s.dtype == torch.float64 and n.dtype == torch.int32
        s, R, t, n = _np(s), _np(R), _np(t), _np(n)
        sr, Rr, tr, nr = rr.minimal(X, Y, with_scale)
        assert np.array_equal(n, nr) and n[:8192].all() and not n[8192:].any()
        d = np.maximum(np.maximum(np.abs(s - sr), np.abs(R - Rr).max(axis=(1, 2))), np.abs(t - tr).max(axis=1))
        print(f"with_scale {with_scale}: difference to the oracle: median {np.median(d):.2e}, worst {d.max():.2e}")
        assert d.max() < 1e-8
        assert not s[8192:].any() and not R[8192:].any() and not t[8192:].any()
        if with_scale:
            err = model_error(s[:4096], R[:4096], t[:4096], st, Rt, tt)
            print(f"against the truth: median {np.median(err):.2e}, worst {err.max():.2e}")
            assert err.max() < 1e-9
        else:
            assert (s[:8192] == 1.0).all()


def _agreement(X, Y, thr, seed, with_scale=True, conf=0.9999, max_iters=1000):
    from roma_amd import align_points
    sim = align_points(_dev(X)[None], _dev(Y)[None], thr, with_scale, conf, max_iters, seed=seed, refine=False)
    ref = rr.ransac(X, Y, thr, conf, max_iters, seed, with_scale)
    info, mask = _np(sim.info[0]), _np(sim.mask[0])
    assert bool(sim.ok[0]) and ref["ok"] and info[4] == 1
    assert info[0] == ref["rounds"]
    assert (info[1], info[2]) == (ref["best_h"], ref["best_root"]) or info[3] == ref["best"], (info, ref)
    diff = mask != ref["mask"]
    print(f"winner {info[1:4]} oracle {ref['best_h'], ref['best_root'], ref['best']}, {diff.sum()} rows differ")
    assert diff.mean() <= 1e-3
    if (info[1], info[2]) == (ref["best_h"], ref["best_root"]):
        ds, dR, dt = abs(float(sim.scale[0]) - ref["s"]), np.abs(_np(sim.R[0]) - ref["R"]).max(), np.abs(_np(sim.t[0]) - ref["t"]).max()
        print(f"|ds| {ds:.2e} |dR| {dR:.2e} |dt| {dt:.2e}")
        assert ds < 1e-8 and dR < 1e-8 and dt < 1e-8, (ds, dR, dt)
        # a differing row sits at the threshold: its squared residual is within a relative 1e-4 of thr^2
        r2 = residual((ref["s"], ref["R"], ref["t"]), X, Y) ** 2
        print("differing rows, r^2 / thr^2 - 1:", r2[diff] / thr ** 2 - 1)
        assert (np.abs(r2[diff] / thr ** 2 - 1) < 1e-4).all()
    return sim, ref


@pytest.mark.parametrize("case", AGREEMENT, ids=lambda c: "-".join(str(v) for v in c))
def test_agreement_with_the_oracle(built_lib, case):
    X, Y, truth, (s, R, t), thr = agreement_scene(*case)
    sim, _ = _agreement(X, Y, thr, seed=case[1])
    assert not _np(sim.mask[0])[~truth].any() and abs(float(sim.scale[0]) / s - 1) < 0.05


def test_rigid_fit_returns_scale_exactly_one(built_lib):
    from roma_amd import align_points
    X, Y, truth, (s, R, t), thr = scene(2000, 0.3, 1.0, rng_seed=4)
    sim, ref = _agreement(X, Y, thr, seed=5, with_scale=False)
    assert float(sim.scale[0]) == 1.0 and ref["s"] == 1.0
    full = align_points(_dev(X), _dev(Y), thr, with_scale=False, seed=5)
    assert float(full.scale) == 1.0 and np.array_equal(_np(full.mask), truth)
    assert np.abs(_np(full.R) - R).max() < 1e-3 and np.abs(_np(full.t) - t).max() < 1e-3
    assert abs(np.linalg.det(_np(full.R)) - 1) < 1e-12


def _run(X, Y, thr, counts, seeds, max_iters, conf=0.9999):
    """the tensors of the RANSAC and of the refinement that follows it"""
    from roma_amd import align_points, refine_similarity
    a = align_points(X, Y, thr, True, conf, max_iters, seed=seeds, counts=counts, refine=False)
    b, cost = refine_similarity(a, X, Y, thr, counts=counts, valid=a.ok, return_cost=True)
    return tuple(a) + tuple(b) + (cost,)


def _same(x, y):
    return torch.equal(x, y) if x.dtype != torch.float64 else np.array_equal(_np(x), _np(y), equal_nan=True)


@pytest.mark.parametrize("max_iters", [256, 300])  # one round and two
def test_tails_ragged_counts_and_rows_beyond_counts(built_lib, max_iters):
    from roma_amd import align_points
    X, Y, thr = ragged_batch(np.nan)
    counts, seeds = RAGGED_COUNTS, torch.arange(31, 37)
    conf = 1.0  # the adaptive count never ends the sampling early, except where every row is an inlier (the problem of 4 rows)
    out = _run(_dev(X), _dev(Y), thr, torch.tensor(counts), seeds, max_iters, conf)
    scale, R, t, mask, ok, info = out[:6]
    fs, fR, ft, fmask, fok, finfo, cost = out[6:]
    assert ok.cpu().tolist() == [False, False, True, True, True, True], ok
    assert info[:, 0].cpu().tolist() == ([0, 0, 1, 1, 1, 1] if max_iters == 256 else [0, 0, 1, 2, 2, 2]), info
    assert info[:, 4].cpu().tolist() == [0, 0, 1, 1, 1, 1] and bool((finfo[2:, 3] == 1).all()) and not bool(finfo[:2].any())
    for b, c in enumerate(counts):
        ref = rr.ransac(f32(X[b, :c]), f32(Y[b, :c]), thr, conf, max_iters, 31 + b)
        assert (int(info[b, 0]), int(info[b, 4]), bool(ok[b])) == (ref["rounds"], int(ref["valid"]), ref["ok"]), (b, info[b], ref)
    for x in (scale[:2], R[:2], t[:2], mask[:2], fs[:2], fR[:2], ft[:2], fmask[:2]):
        assert not bool(x.any())
    # rows beyond counts[b] are never read: huge values in their place change nothing
    X2, Y2, _ = ragged_batch(3e38)
    again = _run(_dev(X2), _dev(Y2), thr, torch.tensor(counts), seeds, max_iters, conf)
    assert all(_same(x, y) for x, y in zip(out, again))
    E = align_points(_dev(X), _dev(Y), thr, True, conf, max_iters, seed=seeds, counts=torch.tensor(counts))
    assert torch.equal(E.scale, fs) and torch.equal(E.R, fR) and torch.equal(E.t, ft) and torch.equal(E.ok, ok) and torch.equal(E.mask[2:], fmask[2:])
    for b, c in enumerate(counts):
        assert not bool(mask[b, c:].any()) and not bool(fmask[b, c:].any())
        if c < 4:  # no problem of fewer than four rows is sampled: nothing to compare beyond the zeros above
            continue
        one = _run(_dev(X[b:b + 1, :c]), _dev(Y[b:b + 1, :c]), thr, None, int(seeds[b]), max_iters, conf)
        for x, y in zip(out, one):
            assert _same(x[b:b + 1, :c] if x.dim() == 2 and x.shape[1] == 257 else x[b:b + 1], y), (b, c)
    # the single-problem form: a model for the problems that have one, None otherwise
    assert align_points(_dev(X[1, :3]), _dev(Y[1, :3]), thr, seed=32) is None
    S = align_points(_dev(X[5]), _dev(Y[5]), thr, True, conf, max_iters, seed=36)
    assert torch.equal(S.R, fR[5]) and torch.equal(S.t, ft[5]) and torch.equal(S.scale, fs[5]) and torch.equal(S.mask, fmask[5]) and tuple(S.t.shape) == (3,)


def test_determinism_and_independence_of_the_batch(built_lib):
    scenes = [scene(700, f, s, rng_seed=k) for f, s, k in ((0.2, 1.0, 1), (0.4, 0.37, 2), (0.1, 2.9, 3), (0.5, 1.0, 4))]
    # one threshold per call: the problems of other scales are posed in the units of the first
    X = _dev(np.stack([sc[0] for sc in scenes]))
    Y = _dev(np.stack([sc[1] / sc[3][0] for sc in scenes]))
    thr = scenes[0][4]
    seeds = torch.tensor([11, 12, 13, 14])
    out = _run(X, Y, thr, None, seeds, 600)
    assert bool(out[4].all()) and bool((out[11][:, 0] > 0).all())
    again = _run(X, Y, thr, None, seeds, 600)
    assert all(_same(x, y) for x, y in zip(out, again))
    perm = [2, 0, 3, 1]
    moved = _run(X[perm], Y[perm], thr, None, seeds[perm], 600)
    assert all(_same(x[perm], y) for x, y in zip(out, moved))
    for b in range(4):
        one = _run(X[b:b + 1], Y[b:b + 1], thr, None, seeds[b:b + 1], 600)
        assert all(_same(x[b:b + 1], y) for x, y in zip(out, one)), b


def test_refinement_matches_the_oracle(built_lib):
    from roma_amd import fit_similarity, refine_similarity
    worst = 0.0
    for seed in REFINE_SEEDS:
        X, Y, truth, model, thr = scene(2000, 0.3, 2.9, rng_seed=10 + seed)
        r = rr.ransac(X, Y, thr, 0.9999, 1000, seed)
        o = rr.refine((r["s"], r["R"], r["t"]), X, Y, thr)
        fit, cost = refine_similarity(_start((r["s"], r["R"], r["t"])), _dev(X), _dev(Y), thr, return_cost=True)
        assert fit.R.dtype == torch.float64 and tuple(fit.t.shape) == (3,) and fit.mask.dtype == torch.bool and fit.info.dtype == torch.int32
        got, cost = fit.info.cpu().tolist(), _np(cost)
        ds, dR, dt = abs(float(fit.scale) - o["s"]), float(np.linalg.norm(_np(fit.R) - o["R"])), float(np.linalg.norm(_np(fit.t) - o["t"]))
        worst = max(worst, ds, dR, dt)
        print(f"seed {seed}: |ds| {ds:.3e} |dR| {dR:.3e} |dt| {dt:.3e} info {got} oracle {o['info']} cost {cost[0]:.6e} -> {cost[1]:.6e}")
        assert got == list(o["info"]) and got[0] >= 1 and bool(fit.ok)
        # rows whose residual sits at the threshold may fall either way; everywhere else the mask is the oracle's
        edge = np.abs(residual((o["s"], o["R"], o["t"]), X, Y) ** 2 / thr ** 2 - 1) < 1e-9
        assert np.array_equal(_np(fit.mask)[~edge], o["mask"][~edge])
        # the truncated cost does not rise, and is the oracle's
        assert cost[1] <= cost[0] and abs(cost[0] / o["cost0"] - 1) < 1e-9 and abs(cost[1] / o["cost"] - 1) < 1e-9
        # no start and no truncation: fit_similarity, which is Umeyama on every row
        free = refine_similarity(None, _dev(X), _dev(Y), math.inf, max_steps=1)
        plain = fit_similarity(_dev(X), _dev(Y))
        assert all(_same(a, b) for a, b in zip(free, plain)) and bool(plain.ok) and plain.info.cpu().tolist() == [1, 2, 2000, 1]
        assert model_error(float(plain.scale), _np(plain.R), _np(plain.t), *umeyama_svd(X, Y)) < 1e-9
    print(f"worst difference {worst:.3e}")
    assert worst <= LM_TOL, worst


def test_refinement_leaves_what_it_cannot_fit(built_lib):
    from roma_amd import refine_similarity
    X, Y, truth, (s, R, t), thr = scene(500, 0.2, 1.0, rng_seed=6)
    ss = np.array([s, s, s])
    Rs = np.stack([R, R, R])
    ts = np.stack([t + [0.2 * thr, 0, 0], t + [0, 0, 100.0], t + [0.2 * thr, 0, 0]])  # problem 1: every row 100 from its partner
    Xb, Yb = _dev(np.stack([X] * 3)), _dev(np.stack([Y] * 3))
    fit, cost = refine_similarity(_start((ss, Rs, ts)), Xb, Yb, thr, valid=torch.tensor([True, True, False]), return_cost=True)
    info = fit.info.cpu().tolist()
    assert info[0][0] >= 1 and info[0][3] == 1 and bool(fit.mask[0].any()) and float(cost[0, 1]) < float(cost[0, 0])
    # a start with no active rows comes back as it went in, and info says so: no step, one cost evaluation, no active row
    assert info[1] == [0, 1, 0, 1] and not bool(fit.mask[1].any()) and float(cost[1, 0]) == float(cost[1, 1])
    assert float(fit.scale[1]) == ss[1] and np.array_equal(_np(fit.R[1]), Rs[1]) and np.array_equal(_np(fit.t[1]), ts[1])
    # a problem that is not valid is untouched
    assert info[2] == [0, 0, 0, 0] and not bool(fit.mask[2].any()) and bool(torch.isnan(cost[2]).all())
    assert float(fit.scale[2]) == ss[2] and np.array_equal(_np(fit.R[2]), Rs[2]) and np.array_equal(_np(fit.t[2]), ts[2])
    assert fit.ok.cpu().tolist() == [True, True, False]


@pytest.mark.parametrize("n", [1, 255, 257])
def test_apply_similarity_against_its_restatement(built_lib, n):
    from roma_amd import apply_similarity
    from registration_cases import rotation
    g = np.random.default_rng(n)
    B, V = 3, 5
    s, R, t = g.uniform(0.3, 3, B), np.stack([rotation(g) for _ in range(B)]), g.uniform(-1e3, 1e3, (B, 3))
    pts = (g.normal(size=(B, n, 3)) * 50).astype(np.float32)
    pts[0, 0, 1] = np.nan
    pts[B - 1, n - 1] = np.inf
    cR, ct = np.stack([[rotation(g, 0.5) for _ in range(V)] for _ in range(B)]), g.uniform(-2, 2, (B, V, 3))
    sim = _start((s, R, t))
    moved, mR, mt = apply_similarity(sim, points=_dev(pts), R=_dev(cR, np.float64), t=_dev(ct, np.float64))
    assert moved.dtype == torch.float32 and tuple(moved.shape) == (B, n, 3) and mR.dtype == torch.float64 and tuple(mt.shape) == (B, V, 3)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(_np(moved[b]), rr.apply_points(s[b], R[b], t[b], pts[b]), equal_nan=True), b
        rR, rt = rr.apply_cameras(s[b], R[b], t[b], cR[b], ct[b])
        assert np.array_equal(_np(mR[b]), rR) and np.array_equal(_np(mt[b]), rt), b
    assert np.isnan(_np(moved[0, 0])).any() and np.isfinite(_np(moved[0, 1:])).all()
    # either half alone, and the single form
    assert torch.equal(apply_similarity(sim, points=_dev(pts)).nan_to_num(1.0), moved.nan_to_num(1.0))
    oR, ot = apply_similarity(sim, R=_dev(cR, np.float64), t=_dev(ct, np.float64))
    assert torch.equal(oR, mR) and torch.equal(ot, mt)
    one = apply_similarity(tuple(v[1] for v in sim), points=_dev(pts[1]))
    assert torch.equal(one, moved[1])


@pytest.mark.parametrize("step", [1, 3])
def test_depth_rows_against_its_restatement(built_lib, step):
    from roma_amd import depth_rows
    d = depth_case()
    D = lambda v: _dev(v, np.float64)  # noqa: E731
    src, dst = depth_rows(_dev(d["da"]), _dev(d["db"]), d["K"], (D(d["Ra"]), D(d["ta"])), (D(d["Rb"]), D(d["tb"])), step)
    rs, rd = rr.depth_rows(d["da"], d["db"], d["K"], d["Ra"], d["ta"], d["Rb"], d["tb"], step)
    assert src.dtype == torch.float32 and tuple(src.shape) == rs.shape and np.isnan(rs).any()
    assert np.array_equal(_np(src), rs, equal_nan=True) and np.array_equal(_np(dst), rd, equal_nan=True)
    # batched: the second problem with the maps exchanged
    da2, db2 = np.stack([d["da"], d["db"]]), np.stack([d["db"], d["da"]])
    Ra2, ta2, Rb2, tb2 = np.stack([d["Ra"], d["Rb"]]), np.stack([d["ta"], d["tb"]]), np.stack([d["Rb"], d["Ra"]]), np.stack([d["tb"], d["ta"]])
    s2, d2 = depth_rows(_dev(da2), _dev(db2), d["K"], (D(Ra2), D(ta2)), (D(Rb2), D(tb2)), step)
    assert np.array_equal(_np(s2[0]), rs, equal_nan=True) and np.array_equal(_np(d2[0]), rd, equal_nan=True)
    assert np.array_equal(_np(s2[1]), rd, equal_nan=True) and np.array_equal(_np(d2[1]), rs, equal_nan=True)


def test_register_depth_maps_recovers_the_similarity(built_lib):
    """Two closed-form depth maps of one view in gauges that differ by a known similarity.  The tolerance, from the f32 rounding
    alone (u = 2^-24, nothing else is inexact: the maps are noise-free and every row is an inlier, so the refinement ends at the
    least-squares fit of all rows).  A row of dst is moved by the rounding of depth_a (u z_a along the ray) and of its three
    stored coordinates (sqrt 3 u max |dst|); a row of src likewise, times s in dst's units: delta = u (z_a + sqrt 3 max |dst|) +
    s u (z_b + sqrt 3 max |src|).  If every row moves by at most delta, the least-squares rotation turns by at most delta / r_min,
    r_min the smallest principal standard deviation of the rows (the relief is thin along the view, that is the weak axis), the
    relative scale moves by at most delta / r_rms <= delta / r_min, and t = yb - s R xb by delta plus the lever of the centroid,
    |xb| s times the sum of both.  Doubled for the second-order terms."""
    from roma_amd import register_depth_maps
    d = depth_case(H=120, W=160)
    s, R, t = d["sim"]
    D = lambda v: _dev(v, np.float64)  # noqa: E731
    sim = register_depth_maps(_dev(d["da"]), _dev(d["db"]), d["K"], (D(d["Ra"]), D(d["ta"])), (D(d["Rb"]), D(d["tb"])), 1e-3, step=4, seed=1)
    assert sim is not None and bool(sim.ok)
    src, dst = rr.depth_rows(d["da"], d["db"], d["K"], d["Ra"], d["ta"], d["Rb"], d["tb"], 4)
    fin = np.isfinite(src).all(axis=1)
    assert np.array_equal(_np(sim.mask), fin)
    src, dst = src[fin].astype(np.float64), dst[fin].astype(np.float64)
    u = 2.0 ** -24
    delta = u * (np.nanmax(d["da"]) + math.sqrt(3) * np.abs(dst).max()) + s * u * (np.nanmax(d["db"]) + math.sqrt(3) * np.abs(src).max())
    r_min = math.sqrt(np.linalg.eigvalsh(np.cov(dst.T))[0])
    lever = np.linalg.norm(src.mean(axis=0)) * s
    tol_R = 2 * delta / r_min
    tol_t = 2 * (delta + lever * 2 * delta / r_min)
    ds, dR, dt = abs(float(sim.scale) / s - 1), np.abs(_np(sim.R) - R).max(), np.abs(_np(sim.t) - t).max()
    print(f"delta {delta:.2e} r_min {r_min:.3f}: |ds|/s {ds:.2e} |dR| {dR:.2e} (tolerance {tol_R:.2e}), |dt| {dt:.2e} (tolerance {tol_t:.2e})")
    assert ds <= tol_R and dR <= tol_R and dt <= tol_t


def test_trajectory_error_against_its_restatement(built_lib):
    from roma_amd import trajectory_error
    D = lambda v: _dev(v, np.float64)  # noqa: E731
    for V, masked in ((3, None), (8, 5), (8, None)):
        R, t, Rg, tg, sim = trajectory_case(V, seed=V)
        ok = np.ones(V, dtype=bool)
        if masked is not None:
            ok[masked] = False
        e = trajectory_error(D(R), D(t), D(Rg), D(tg), None if masked is None else torch.as_tensor(ok, device=DEV))
        ref = rr.trajectory_error(R, t, Rg, tg, ok)
        assert bool(e.ok) and ref["ok"] and e.rmse.dtype == torch.float64 and tuple(e.centre_err.shape) == (V,)
        diffs = [abs(float(e.scale) - ref["s"]), np.linalg.norm(_np(e.R) - ref["R"]), np.linalg.norm(_np(e.t) - ref["t"]),
                 np.abs(_np(e.centre_err) - ref["centre_err"]).max(), np.abs(_np(e.rot_err_deg) - ref["rot_err_deg"]).max(),
                 abs(float(e.rmse) - ref["rmse"])]
        print(f"V {V} masked {masked}: rmse {float(e.rmse):.4f}, differences {['%.1e' % v for v in diffs]}")
        assert max(diffs) <= LM_TOL, diffs
    # fewer than three usable views, a collinear path, and a batch of both next to a good one
    R3, t3, Rg3, tg3, _ = trajectory_case(3, seed=3)
    few = trajectory_error(D(R3), D(t3), D(Rg3), D(tg3), torch.tensor([True, False, True], device=DEV))
    assert not bool(few.ok) and math.isnan(float(few.rmse)) and bool(torch.isnan(few.centre_err).all()) and bool(torch.isnan(few.R).all())
    Rc, tc, Rgc, tgc, _ = trajectory_case(8, seed=9, collinear=True)
    R8, t8, Rg8, tg8, _ = trajectory_case(8, seed=8)
    both = trajectory_error(D(np.stack([Rc, R8])), D(np.stack([tc, t8])), D(np.stack([Rgc, Rg8])), D(np.stack([tgc, tg8])))
    assert both.ok.cpu().tolist() == [False, True] and bool(torch.isnan(both.rot_err_deg[0]).all()) and bool(torch.isnan(both.scale[0]))
    alone = trajectory_error(D(R8), D(t8), D(Rg8), D(tg8))
    assert all(_same(a[1], b) for a, b in zip(both, alone))
    rigid = trajectory_error(D(R8), D(t8), D(Rg8), D(tg8), with_scale=False)
    assert float(rigid.scale) == 1.0 and float(rigid.rmse) > float(alone.rmse)


def _angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def test_two_reconstructions_joined_by_one_similarity(built_lib):
    """Six views of one scene, reconstructed as views {0, 1, 2, 3} (a) and {2, 3, 4, 5} (b): each in its own gauge.  The shared
    tracks' points give the similarity b -> a; b's cameras of views 2 and 3, moved by it, must be a's own."""
    from roma_amd import align_points, apply_similarity, reconstruct_views
    from views_cases import NORM_THR, THR, scene as views_scene
    s = views_scene(6, 300, 5, missing=0.2, noise_px=0.5, outlier_frac=0.05)
    kp = np.asarray(s["kpts"], dtype=np.float32)
    va, vb = [0, 1, 2, 3], [2, 3, 4, 5]
    ra = reconstruct_views(_dev(kp[va]), s["K"][va], NORM_THR, THR, seed=3)
    rb = reconstruct_views(_dev(kp[vb]), s["K"][vb], NORM_THR, THR, seed=3)
    assert bool(ra.ok) and bool(rb.ok) and bool(ra.view_ok.all()) and bool(rb.view_ok.all())
    thresh = 0.2  # in a's units: its seed baseline is 1 and the relief lies 6 to 10 away
    Pb, Pa = rb.points.to(torch.float32), ra.points.to(torch.float32)  # NaN rows stay in place
    sim = align_points(Pb, Pa, thresh, seed=7)
    assert sim is not None and int(sim.mask.sum()) >= 50
    mR, mt = apply_similarity(sim, R=rb.R, t=rb.t)
    # the reference on the same device outputs
    xb, xa = _np(Pb).astype(np.float64), _np(Pa).astype(np.float64)
    ref = rr.align_points(xb, xa, thresh, seed=7)
    ds, dR, dt = abs(float(sim.scale) - ref["s"]), np.abs(_np(sim.R) - ref["R"]).max(), np.abs(_np(sim.t) - ref["t"]).max()
    print(f"against the reference: |ds| {ds:.2e} |dR| {dR:.2e} |dt| {dt:.2e}, masks differ in {(ref['mask'] != _np(sim.mask)).sum()} rows")
    assert max(ds, dR, dt) < 1e-8 and (ref["mask"] != _np(sim.mask)).mean() <= 1e-3
    rR, rt = rr.apply_cameras(float(sim.scale), _np(sim.R), _np(sim.t), _np(rb.R), _np(rb.t))
    assert np.array_equal(_np(mR), rR) and np.array_equal(_np(mt), rt)
    # against a's own cameras, with numpy Umeyama on the rows whose observations are all true as the yardstick
    clean = (s["truth"] | np.isnan(s["kpts"]).any(axis=2)).all(axis=0) & np.isfinite(xa).all(axis=1) & np.isfinite(xb).all(axis=1)
    us, uR, ut = umeyama_svd(xb[clean], xa[clean])
    eR, et = rr.apply_cameras(us, uR, ut, _np(rb.R), _np(rb.t))
    Ra, ta = _np(ra.R), _np(ra.t)
    for k in (0, 1):  # b's views 0 and 1 are a's views 2 and 3
        centre = lambda Rc, tc: -Rc.T @ tc  # noqa: E731
        d_R, e_R = _angle_deg(_np(mR)[k], Ra[2 + k]), _angle_deg(eR[k], Ra[2 + k])
        d_c, e_c = np.linalg.norm(centre(_np(mR)[k], _np(mt)[k]) - centre(Ra[2 + k], ta[2 + k])), np.linalg.norm(centre(eR[k], et[k]) - centre(Ra[2 + k], ta[2 + k]))
        print(f"view {2 + k}: rotation {d_R:.4f} degrees (Umeyama {e_R:.4f}), centre {d_c:.4e} (Umeyama {e_c:.4e})")
        assert d_R <= 2 * e_R and d_c <= 2 * e_c
