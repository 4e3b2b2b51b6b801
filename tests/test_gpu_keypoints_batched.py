"""roma_amd.match_keypoints / RegressionMatcher.match_keypoints_batched (roma_op_match_keypoints, csrc/keypoints_batched.hip) on the
cases of tests/keypoints_cases.py: index-exact against the numpy restatement tools/keypoints_ref.py, the reference's goldens and the
single-pair match_keypoints; the sampled stage bit-equal to roma_op_sample_warp_at; independence of batch size, position, padding
width, padding content and run; the cap, views, strides, pixel sizes, the single-pair forms and the chain into find_homography."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import keypoints_cases as cases
from test_cpu_keypoints_batched import CAP_M
from test_cpu_model_refine import corner_error

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = ("kpts_A", "kpts_B", "inds", "counts", "total")


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cases are read-only


def run(b, stages=False, **kw):
    """one call on a batch of numpy arrays (keypoints_cases.batch); the KeypointMatches as a dict of numpy arrays"""
    import roma_amd
    kw.setdefault("max_matches", cases.NB)
    out = roma_amd.match_keypoints(dev(b["x_A"]), dev(b["x_B"]), dev(b["warp"]), dev(b["cert"]), dev(b["counts_A"]), dev(b["counts_B"]),
                                   _stages=stages, **kw)
    torch.cuda.synchronize()
    if stages:
        return dict(zip(FIELDS, (o.cpu().numpy() for o in out[0]))), tuple(o.cpu().numpy() for o in out[1])
    return dict(zip(FIELDS, (o.cpu().numpy() for o in out)))


@functools.lru_cache(maxsize=None)
def base(params):
    """the seven pairs in one call, computed once per parameter set"""
    return run(cases.batch(), **cases.PARAMS[params])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(same_bits(a[k][rows_a], b[k][rows_b]) for k in FIELDS)


def check_pair(out, k, x_a, x_b, e, M):
    """row k of a result against the pairs e [n, 2] of that pair: counts, indices, gathered keypoints, padding"""
    n = min(len(e), M)
    assert out["total"].dtype == np.int64 and out["counts"].dtype == np.int32 and out["inds"].dtype == np.int32
    assert int(out["total"][k]) == len(e) and int(out["counts"][k]) == n, (k, int(out["total"][k]), len(e))
    assert np.array_equal(out["inds"][k, :n], e[:n]) and np.all(out["inds"][k, n:] == -1), k
    assert same_bits(out["kpts_A"][k, :n], np.asarray(x_a)[e[:n, 0]]) and same_bits(out["kpts_B"][k, :n], np.asarray(x_b)[e[:n, 1]]), k
    assert same_bits(out["kpts_A"][k, n:], np.zeros((M - n, 2), np.float32)) and same_bits(out["kpts_B"][k, n:], np.zeros((M - n, 2), np.float32)), k


def single_pair(x_a, x_b, warp, cert, **kw):
    """the existing single-pair RegressionMatcher.match_keypoints on the pair's own unpadded tensors, as [n, 2] int64"""
    from roma_amd.matcher import RegressionMatcher
    i, j = RegressionMatcher.__new__(RegressionMatcher).match_keypoints(dev(x_a), dev(x_b), dev(warp), dev(cert), return_inds=True, **kw)
    return np.stack([i.cpu().numpy(), j.cpu().numpy()], axis=-1).astype(np.int64)


# ------------------------------------------------------------------------------------------------- against the three references
@pytest.mark.parametrize("params", list(cases.PARAMS))
def test_batch_is_index_exact(params):
    out = base(params)
    assert out["inds"].shape == (7, cases.NB, 2) and out["kpts_A"].shape == out["kpts_B"].shape == (7, cases.NB, 2)
    for k, (x_a, x_b, warp, cert) in enumerate(cases.pairs()):
        e = cases.expected(k, params)
        print(f"pair {k} ({params}): {int(out['total'][k])} pairs, expected {len(e)}")
        check_pair(out, k, x_a, x_b, e, cases.NB)
        assert np.array_equal(single_pair(x_a, x_b, warp, cert, **cases.PARAMS[params]), e), k
    assert np.array_equal(out["inds"][0, :out["counts"][0]], cases.golden_inds("keypoints", params))
    assert np.array_equal(out["inds"][1, :out["counts"][1]], cases.golden_inds("keypoints_ties", params))
    assert out["total"].tolist()[:3] == [cases.PAIRS[k][params] for k in range(3)] and out["total"].tolist()[4:6] == [0, 0]


@pytest.mark.parametrize("params", list(cases.PARAMS))
def test_generated_case_crosses_tiles_and_slices(params):
    x_a, x_b, warp, cert = cases.generated()
    e = cases.expected("generated", params)
    assert len(e) == cases.PAIRS["generated"][params]
    b = dict(x_A=x_a[None], x_B=x_b[None], warp=warp[None], cert=cert[None], counts_A=np.array([1300], np.int32), counts_B=np.array([2100], np.int32))
    out = run(b, max_matches=None, **cases.PARAMS[params])
    assert out["inds"].shape == (1, 2100, 2)  # max_matches defaults to max(NA, NB)
    check_pair(out, 0, x_a, x_b, e, 2100)
    assert np.array_equal(single_pair(x_a, x_b, warp, cert, **cases.PARAMS[params]), e)
    # in a batch of three behind two smaller pairs, padded to 2304 x 3072: the slices fall elsewhere, the result does not move
    wide = cases.batch(order=(1, 2, "generated"), na_pad=2304, nb_pad=3072, fill=np.nan)
    out3 = run(wide, max_matches=2100, **cases.PARAMS[params])
    assert same_result(out3, out, slice(2, 3), slice(0, 1))
    check_pair(out3, 0, *cases.pairs()[1][:2], cases.expected(1, params), 2100)


def test_sampled_stage_has_the_bits_of_sample_warp_at():
    from roma_amd import _lib
    lib = _lib.load()
    b = cases.batch()
    _, (p, c) = run(b, stages=True)
    assert p.shape == (7, cases.NA, 2) and c.shape == (7, cases.NA) and p.dtype == c.dtype == np.float32
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for k, (x_a, _, warp, cert) in enumerate(cases.pairs()):
        na = len(x_a)
        if na == 0:
            continue
        w, ce, xa = dev(warp), dev(cert), dev(x_a)
        ref_p, ref_c = torch.empty((na, 2), device=DEV), torch.empty((na,), device=DEV)
        with torch.cuda.device(DEV):
            _lib.check(lib.roma_op_sample_warp_at(P(w), P(ce), 96, 128, P(xa), na, P(ref_p), P(ref_c), stream))
        torch.cuda.synchronize()
        assert same_bits(p[k, :na], ref_p.cpu().numpy()) and same_bits(c[k, :na], ref_c.cpu().numpy()), k
        _, _, rp, rc = cases.checked(k, "default")  # the restatement does not fuse: close, not equal
        assert np.abs(p[k, :na] - rp).max() < 1e-6 and np.abs(c[k, :na] - rc).max() < 1e-6


# ------------------------------------------------------------------------------------------------- a pair's result is its own
@pytest.mark.parametrize("params", list(cases.PARAMS))
def test_result_does_not_depend_on_batch_size_position_or_padding_width(params):
    full = base(params)
    kw = cases.PARAMS[params]
    for k in range(7):  # B = 1
        assert same_result(run(cases.batch(order=(k,)), **kw), full, slice(0, 1), slice(k, k + 1)), k
    rev = run(cases.batch(order=tuple(range(6, -1, -1))), **kw)
    assert all(same_bits(rev[f][::-1], full[f]) for f in FIELDS)
    for na_pad, nb_pad in ((1024, 2048), (701, 4097)):  # wider: other slice boundaries; M stays
        assert same_result(run(cases.batch(na_pad=na_pad, nb_pad=nb_pad), **kw), full), (na_pad, nb_pad)


def test_rows_beyond_the_counts_are_not_read_and_runs_repeat():
    full = base("default")
    assert same_result(run(cases.batch()), full)  # a second run
    for fill in (np.nan, 1e30):
        assert same_result(run(cases.batch(fill=fill)), full), fill
    # device-side counts beyond the padded width are clamped to it
    b = cases.batch(order=(0, 0))
    b["counts_A"], b["counts_B"] = np.array([700, 5000], np.int32), np.array([900, 1 << 30], np.int32)
    out = run(b)
    assert same_result(out, full, slice(0, 1), slice(0, 1)) and same_result(out, full, slice(1, 2), slice(0, 1))
    b["counts_A"], b["counts_B"] = np.array([-3, 700], np.int32), np.array([900, -1], np.int32)  # and below zero: empty
    out = run(b)
    assert out["total"].tolist() == [0, 0] and out["counts"].tolist() == [0, 0] and np.all(out["inds"] == -1) and not out["kpts_A"].any()


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_max_matches_caps_the_rows_and_not_the_total(fmt):
    order = ("ties_matched", 2, 0)
    b = cases.batch(order=order)
    exp = [cases.expected(c, "default") for c in order]
    assert len(exp[0]) > b["counts_A"][0]  # more pairs than rows of A
    free = run(b)
    for k in range(3):
        check_pair(free, k, b["x_A"][k], b["x_B"][k], exp[k], cases.NB)
    cap = run(b, max_matches=CAP_M)
    assert cap["inds"].shape == (3, CAP_M, 2)
    assert cap["counts"].tolist() == [CAP_M, len(exp[1]), CAP_M] and cap["total"].tolist() == [len(e) for e in exp] == free["total"].tolist()
    for k in range(3):  # the first M in row-major order; a row written past a pair's M would land in the next pair's
        check_pair(cap, k, b["x_A"][k], b["x_B"][k], exp[k], CAP_M)
        assert all(same_bits(cap[f][k], free[f][k, :CAP_M]) for f in FIELDS[:3])
    one = run(b, max_matches=1)
    assert one["counts"].tolist() == [1, 1, 1] and np.array_equal(one["inds"][:, 0], np.stack([e[0] for e in exp]))
    # and past the last pair's: the C entry point (of either build) on outputs with 64 spare rows behind them
    from roma_amd import _lib
    lib = _lib.load(fmt)
    t = {k: dev(v) for k, v in b.items()}
    spare = 64
    inds = torch.full((3 * CAP_M + spare, 2), 77, device=DEV, dtype=torch.int32)
    ka, kb = torch.full((3 * CAP_M + spare, 2), 77.0, device=DEV), torch.full((3 * CAP_M + spare, 2), 77.0, device=DEV)
    counts, total = torch.zeros(3, device=DEV, dtype=torch.int32), torch.zeros(3, device=DEV, dtype=torch.int64)
    need = lib.roma_op_match_keypoints_workspace(3, cases.NA, cases.NB)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    with torch.cuda.device(DEV):
        _lib.check(lib.roma_op_match_keypoints(P(t["x_A"]), P(t["x_B"]), P(t["counts_A"]), P(t["counts_B"]), P(t["warp"]), 96 * 128 * 4, 128 * 4,
                                               P(t["cert"]), 96 * 128, 128, None, 0, 3, cases.NA, cases.NB, 96, 128, 0.005, 0.0, CAP_M, P(inds), P(ka),
                                               P(kb), P(counts), P(total), P(ws), need, C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)))
    torch.cuda.synchronize()
    assert same_bits(inds[:3 * CAP_M].cpu().numpy().reshape(3, CAP_M, 2), cap["inds"]) and bool((inds[3 * CAP_M:] == 77).all())
    assert same_bits(ka[:3 * CAP_M].cpu().numpy().reshape(3, CAP_M, 2), cap["kpts_A"]) and bool((ka[3 * CAP_M:] == 77).all())
    assert same_bits(kb[:3 * CAP_M].cpu().numpy().reshape(3, CAP_M, 2), cap["kpts_B"]) and bool((kb[3 * CAP_M:] == 77).all())
    assert counts.tolist() == cap["counts"].tolist() and total.tolist() == cap["total"].tolist()


def test_symmetric_view_strides_and_matcher_method():
    import roma_amd
    from roma_amd.matcher import RegressionMatcher
    full = base("loose")
    b = cases.batch()
    kw = dict(max_matches=cases.NB, **cases.PARAMS["loose"])
    args = [dev(b[k]) for k in ("x_A", "x_B", "warp", "cert", "counts_A", "counts_B")]
    rng = np.random.default_rng(0)
    # the A -> B half of a symmetric warp, read in place, against an explicit copy of it
    sym_w = torch.cat([args[2], dev(rng.standard_normal((7, 96, 128, 4)).astype(np.float32))], dim=2)
    sym_c = torch.cat([args[3], dev(rng.random((7, 96, 128)).astype(np.float32))], dim=2)
    got = roma_amd.match_keypoints(args[0], args[1], sym_w, sym_c, args[4], args[5], symmetric=True, **kw)
    copy = roma_amd.match_keypoints(args[0], args[1], sym_w[:, :, :128].contiguous(), sym_c[:, :, :128].contiguous(), args[4], args[5], **kw)
    via = RegressionMatcher.__new__(RegressionMatcher).match_keypoints_batched(args[0], args[1], sym_w, sym_c, args[4], args[5], symmetric=True, **kw)
    # strided everything: warp and certainty inside larger allocations, keypoints as columns of wider rows, int64 counts
    big_w = torch.full((7, 99, 131, 4), float("nan"), device=DEV)
    big_c = torch.full((7, 99, 131), float("nan"), device=DEV)
    big_w[:, 2:98, :128], big_c[:, 2:98, 3:] = args[2], args[3]
    xa4 = torch.full((7, cases.NA, 4), float("nan"), device=DEV)
    xb4 = torch.full((7, cases.NB, 4), float("nan"), device=DEV)
    xa4[..., :2], xb4[..., 2:] = args[0], args[1]
    strided = roma_amd.match_keypoints(xa4[..., :2], xb4[..., 2:], big_w[:, 2:98, :128], big_c[:, 2:98, 3:], args[4].long(), args[5].long(), **kw)
    torch.cuda.synchronize()
    for name, r in (("symmetric", got), ("copy", copy), ("method", via), ("strided", strided)):
        assert isinstance(r, roma_amd.KeypointMatches)
        assert same_result(dict(zip(FIELDS, (o.cpu().numpy() for o in r))), full), name


def test_sizes_give_the_bits_of_to_pixel_coordinates():
    from roma_amd.matcher import RegressionMatcher
    full = base("default")
    m = RegressionMatcher.__new__(RegressionMatcher)
    scal = (479, 641, 1080, 1920)
    out = run(cases.batch(), sizes=scal)
    per = np.array([[480 + 7 * k, 640 - 3 * k, 333 + k, 1001 + 2 * k] for k in range(7)])
    out_t = run(cases.batch(), sizes=dev(per.astype(np.float32)))
    out_i = run(cases.batch(), sizes=dev(per))  # an integer tensor is taken as well
    for k in range(7):
        n = int(full["counts"][k])
        for o, (ha, wa, hb, wb) in ((out, scal), (out_t, per[k].tolist()), (out_i, per[k].tolist())):
            assert same_bits(o["inds"][k], full["inds"][k]) and o["counts"][k] == n and o["total"][k] == full["total"][k]
            ka, kb = m.to_pixel_coordinates(torch.from_numpy(np.concatenate([full["kpts_A"][k, :n], full["kpts_B"][k, :n]], -1)), ha, wa, hb, wb)
            assert same_bits(o["kpts_A"][k, :n], ka.numpy()) and same_bits(o["kpts_B"][k, :n], kb.numpy()), k
            assert not o["kpts_A"][k, n:].any() and not o["kpts_B"][k, n:].any()


def test_single_pair_forms():
    import roma_amd
    full = base("default")
    for k in (1, 2, 4, 5):
        x_a, x_b, warp, cert = cases.pairs()[k]
        r = roma_amd.match_keypoints(dev(x_a.reshape(-1, 2)), dev(x_b.reshape(-1, 2)), dev(warp), dev(cert))
        torch.cuda.synchronize()
        M = max(len(x_a), len(x_b))
        assert r.inds.shape == (M, 2) and r.kpts_A.shape == r.kpts_B.shape == (M, 2) and r.counts.shape == r.total.shape == ()
        n = int(r.counts)
        assert n == int(full["counts"][k]) == int(r.total)
        assert np.array_equal(r.inds.cpu().numpy()[:n], full["inds"][k, :n]) and bool((r.inds[n:] == -1).all())
        assert same_bits(r.kpts_A.cpu().numpy()[:n], full["kpts_A"][k, :n]) and same_bits(r.kpts_B.cpu().numpy()[:n], full["kpts_B"][k, :n])


# ------------------------------------------------------------------------------------------------- into the batched geometry
def test_chain_into_batched_homography():
    """detector keypoints on a synthetic dense warp of a known homography: keypoints of A, their transfers with a little noise plus
    outliers as keypoints of B -> match_keypoints(sizes=...) -> find_homography(counts=m.counts); the second pair has fewer
    keypoints, so fewer matches than M: its tail is padding that counts must keep out of the fit"""
    import roma_amd
    Hh, Ww, size, NA_, NB_ = 48, 48, 480, 600, 800
    Hs = np.array([[[1.05, 0.03, 12.0], [-0.02, 0.98, -7.0], [2e-5, -1e-5, 1.0]],
                   [[0.93, -0.06, 30.0], [0.05, 1.02, 9.0], [-3e-5, 2e-5, 1.0]]])
    g = (np.arange(Hh) + 0.5) / Hh * 2 - 1
    grid = np.stack(np.meshgrid(g, g, indexing="xy"), -1)                     # [H, W, 2] normalised (x, y) of image A
    rng = np.random.default_rng(7)
    warp, cert = np.zeros((2, Hh, Ww, 4), np.float32), np.zeros((2, Hh, Ww), np.float32)
    x_A, x_B = np.zeros((2, NA_, 2), np.float32), np.zeros((2, NB_, 2), np.float32)
    counts_A, counts_B = np.array([NA_, 150], np.int32), np.array([NB_, 260], np.int32)

    def transfer(x, Hm):
        pa = np.concatenate([size / 2 * (x + 1), np.ones(x.shape[:-1] + (1,))], -1) @ Hm.T
        return pa[..., :2] / pa[..., 2:] * 2 / size - 1
    for b in range(2):
        xb = transfer(grid, Hs[b])
        warp[b] = np.concatenate([grid, xb], -1)
        cert[b] = (np.abs(xb).max(-1) < 1) * 0.9
        na, nb = int(counts_A[b]), int(counts_B[b])
        x_A[b, :na] = rng.random((na, 2)) * 1.7 - 0.85
        moved = transfer(x_A[b, :na].astype(np.float64), Hs[b]) + rng.standard_normal((na, 2)) * (0.3 * 2 / size)  # 0.3 px of noise
        x_B[b, :nb] = np.concatenate([moved, rng.random((nb - na, 2)) * 2 - 1])[rng.permutation(nb)]     # plus outliers, shuffled
    m = roma_amd.match_keypoints(dev(x_A), dev(x_B), dev(warp), dev(cert), dev(counts_A), dev(counts_B), sizes=(size, size, size, size))
    assert m.kpts_A.shape == (2, NB_, 2) and m.kpts_B.shape == (2, NB_, 2)
    Hd, mask, ok = roma_amd.find_homography(m.kpts_A, m.kpts_B, ransac_reproj_threshold=1.0, seed=1, counts=m.counts)
    torch.cuda.synchronize()
    counts = m.counts.tolist()
    print("matches per pair:", counts, "of", counts_A.tolist(), "keypoints of A")
    assert 400 < counts[0] <= NA_ and 80 < counts[1] <= 150 and counts[1] < NB_
    assert ok.tolist() == [True, True]
    for b in range(2):
        err = corner_error(Hd[b].cpu().numpy(), Hs[b], size)
        print(f"pair {b}: corner error {err:.2e} px, {int(mask[b].sum())} inliers of {counts[b]}")
        assert err < 1.0 and int(mask[b].sum()) > 0.9 * counts[b] and not bool(mask[b, counts[b]:].any())
