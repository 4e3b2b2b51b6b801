"""roma_amd.sample_matches / RegressionMatcher.sample_batched (roma_op_sample_matches, csrc/sample_batched.hip) against its numpy
restatement tools/sample_ref.py, stage by stage: the first draw, the density, the second draw driven by the device's density,
then reproducibility (run to run, batch size, position in the batch), the four sample modes, the distribution against the torch
oracle, and the chain into the batched geometry."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_cpu_model_refine import corner_error
from test_cpu_sample_batched import GAP, K, M, MODES, N, NUM, SEEDS, THRESH, ascending, cut_gaps, oracle, pairs, two_clusters

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sample_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(x, c, seeds, mode="threshold_balanced", num=NUM):
    """(matches, certainty, counts, idx, first_idx, density) of one call, as numpy arrays"""
    import roma_amd
    out = roma_amd.sample_matches(torch.as_tensor(x).to(DEV), torch.as_tensor(c).to(DEV), num=num, sample_mode=mode,
                                  sample_thresh=THRESH, seed=torch.tensor(list(seeds), dtype=torch.int64), return_counts=True,
                                  return_indices=True, _stages=True)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def batch(mode="threshold_balanced"):
    """the four pairs of test_cpu_sample_batched.pairs in one call, computed once per mode"""
    return run(*pairs(), SEEDS, mode)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def thresholded(c, mode="threshold_balanced"):
    return np.where(c > np.float32(THRESH), np.float32(1), c) if "threshold" in mode else c


def check_first_draw(first, o, c):
    """the device's first draw against the oracle's: the same set, provided the oracle's cut is clear of rounding (asserted), in
    ascending order of the oracle's keys; filler rows are the lowest zero-certainty indices, in index order"""
    k = len(first)
    up, down, ties, taken = cut_gaps(o["keys1"], k)
    assert up > GAP and down > GAP, (up, down)
    assert len(set(first.tolist())) == k and set(first.tolist()) == set(o["first_idx"].tolist())
    assert ascending(o["keys1"][first])
    npos = int((c > 0).sum())
    if npos < k:
        assert np.array_equal(first[npos:], np.nonzero(~(c > 0))[0][:k - npos])
    return ties, taken


def test_first_draw_set_order_and_ties():
    x, c = pairs()
    first = batch()[4]
    assert first.shape == (4, K) and first.dtype == np.int64
    for b in range(4):
        o = oracle(b)
        ties, taken = check_first_draw(first[b], o, thresholded(c[b]))
        if b == 1:  # all weights 1: tied keys exist, and one tie sits exactly at the cut - the lower index is in, the higher out
            finite = o["keys1"][np.isfinite(o["keys1"])]
            assert len(np.unique(finite)) < len(finite) and (ties, taken) == (2, 1)
            lo, hi = np.nonzero(o["keys1"] == np.sort(o["keys1"])[K - 1])[0]
            assert lo in first[b] and hi not in first[b] and first[b][-1] == lo
    # k = n: every row, in draw order
    xs, cs = x[:1, :600], c[:1, :600]
    _, _, counts, idx, first, dens = run(xs, cs, SEEDS[:1])
    o = oracle(0, n=600)
    assert first.shape == (1, 600) and sorted(first[0].tolist()) == list(range(600)) and ascending(o["keys1"][first[0]])
    assert idx.shape == (1, 500) and len(set(idx[0].tolist())) == 500 and counts[0] == 500


def test_density_of_the_first_draw():
    """the bound test_kde_vs_reference_golden_and_oracle holds kde to, on K = 2000 rows: two reference slices, the second with a
    ragged tile, and a ragged last query block"""
    x, _ = pairs()
    first, dens = batch()[4], batch()[5]
    assert dens.shape == (4, K) and dens.dtype == np.float32
    for b in range(4):
        ref = sr.density_f64(x[b, first[b]])
        err = np.abs(dens[b] - ref)
        print(f"pair {b}: max |density - f64| / (1e-5 |ref| + 1e-7) = {np.max(err / (1e-5 * np.abs(ref) + 1e-7)):.3f}")
        assert np.all(err <= 1e-5 * np.abs(ref) + 1e-7)


def check_second_draw(b, out, x, c, seed, mode="threshold_balanced"):
    """the device's result against the oracle's second draw over the device's own first draw and density"""
    matches, cert, counts, idx, first, dens = (o[b] for o in out)
    cw = thresholded(c, mode)
    p = sr.balance_weights(dens, cw[first])
    m = len(idx)
    second, keys2 = sr.draw(p, m, seed ^ sr.SECOND_DRAW_SEED)
    up, down, _, _ = cut_gaps(keys2, m)  # one f32 ulp of p moves a key by 1.2e-7 relative
    assert up > GAP and down > GAP, (up, down)
    assert len(set(idx.tolist())) == m and set(idx.tolist()) == set(first[second].tolist())
    row_of = {int(i): j for j, i in enumerate(first)}
    assert ascending(keys2[[row_of[int(i)] for i in idx]])
    assert np.array_equal(matches, x[idx]) and np.array_equal(cert, cw[idx])
    npos = int((cw > 0).sum())
    assert counts == min(m, npos) and np.all(cert[:counts] > 0) and np.all(cert[counts:] == 0)


def test_second_draw_gather_and_counts():
    x, c = pairs()
    out = batch()
    assert out[0].shape == (4, M, 4) and out[1].shape == (4, M) and out[3].shape == (4, M) and out[3].dtype == np.int64
    assert out[2].dtype == np.int32 and out[2].tolist() == [500, 500, 500, 300]
    for b in range(4):
        check_second_draw(b, out, x[b], c[b], SEEDS[b])
    assert np.all(out[1][3, 300:] == 0) and np.all(c[3, out[3][3, 300:]] == 0) and np.all(out[1][3, :300] > 0)
    # k = n = 600
    xs, cs = x[:1, :600], c[:1, :600]
    check_second_draw(0, run(xs, cs, SEEDS[:1]), xs[0], cs[0], SEEDS[0])


def test_reproducible_and_independent_of_the_batch():
    x, c = pairs()
    ref = batch()
    again = run(x, c, SEEDS)
    for a, r in zip(again, ref):
        assert same_bits(a, r)  # bit for bit, the density included
    for b in range(4):  # each pair alone
        alone = run(x[b:b + 1], c[b:b + 1], SEEDS[b:b + 1])
        for a, r in zip(alone, ref):
            assert same_bits(a[0], r[b]), b
    perm = [2, 0, 3, 1]  # the pairs permuted together with their seeds
    moved = run(x[perm], c[perm], [SEEDS[b] for b in perm])
    for a, r in zip(moved, ref):
        assert same_bits(a, r[perm])
    # another seed is another sample
    other = run(x[:1], c[:1], [SEEDS[0] + 1])
    assert not np.array_equal(other[3][0], ref[3][0])


@pytest.mark.parametrize("mode", MODES[1:])
def test_sample_modes(mode):
    x, c = pairs()
    matches, cert, counts, idx, first, dens = out = batch(mode)
    k = K if "balanced" in mode else NUM
    assert matches.shape == (4, M, 4) and cert.shape == (4, M) and idx.shape == (4, M) and first.shape == (4, k)
    for b in range(4):
        cw = thresholded(c[b], mode)
        check_first_draw(first[b], oracle(b, mode), cw)
        if "balanced" in mode:
            check_second_draw(b, out, x[b], c[b], SEEDS[b], mode)
        else:  # the first draw is the result
            assert np.array_equal(idx[b], first[b]) and np.array_equal(matches[b], x[b, idx[b]]) and np.array_equal(cert[b], cw[idx[b]])
            assert counts[b] == min(M, int((cw > 0).sum()))
        vals = set(np.unique(cert[b]).tolist())
        raw = set(np.unique(c[b]).tolist())
        assert vals <= ({1.0} | {v for v in raw if v <= np.float32(THRESH)} if "threshold" in mode else raw)
    assert (1.0 in set(np.unique(cert).tolist())) == ("threshold" in mode)


def test_distribution_matches_the_torch_oracle():
    """test_sample_distribution_matches_oracle's scene, statistic, tolerance and four draws - the four draws as one batch"""
    from oracle import roma_oracle as O
    x, c = two_clusters()
    matches = run(np.stack([x] * 4), np.stack([c] * 4), (11, 12, 13, 14))[0]
    fr = [float((matches[b, :, 0] < -0.1).mean()) for b in range(4)]
    gen = torch.Generator().manual_seed(3)
    fo = []
    for _ in range(4):
        om, _ = O.sample(torch.from_numpy(x), torch.from_numpy(c), num=500, generator=gen)
        fo.append(float((om[:, 0] < -0.1).float().mean()))
    assert abs(np.mean(fr) - np.mean(fo)) < 0.08, (fr, fo)
    assert np.mean(fr) > 0.5


def test_python_forms_and_seeds():
    import roma_amd
    from roma_amd.matcher import RegressionMatcher
    x, c = pairs()
    ref = batch()
    xd, cd = torch.as_tensor(x).to(DEV), torch.as_tensor(c).to(DEV)
    seeds = torch.tensor(SEEDS, dtype=torch.int64)
    m = RegressionMatcher.__new__(RegressionMatcher)  # sample_batched() needs only the two sampling attributes
    m.sample_mode, m.sample_thresh = "threshold_balanced", THRESH
    gm, gc = m.sample_batched(xd.reshape(4, 40, 100, 4), cd.reshape(4, 40, 100), num=NUM, seed=seeds)  # [B, H, W, 4]
    assert gm.shape == (4, M, 4) and gc.shape == (4, M) and gm.is_cuda and gm.dtype == torch.float32
    assert np.array_equal(gm.cpu().numpy(), ref[0]) and np.array_equal(gc.cpu().numpy(), ref[1])
    gm, gc, counts, idx = roma_amd.sample_matches(xd[1], cd[1], num=NUM, sample_thresh=THRESH, seed=SEEDS[1], return_counts=True,
                                                  return_indices=True)                                           # [n, 4]: one pair
    assert gm.shape == (M, 4) and gc.shape == (M,) and counts.shape == () and idx.shape == (M,)
    assert np.array_equal(idx.cpu().numpy(), ref[3][1]) and int(counts) == 500
    gm2, _ = roma_amd.sample_matches(xd[1].reshape(40, 100, 4), cd[1].reshape(40, 100), num=NUM, sample_thresh=THRESH, seed=SEEDS[1],
                                     batched=False)                                                              # [H, W, 4]
    assert torch.equal(gm2, gm)
    torch.manual_seed(5)   # seed=None: from torch's CPU generator, one seed per pair
    a = roma_amd.sample_matches(xd, cd, num=NUM, sample_thresh=THRESH, return_indices=True)[2]
    torch.manual_seed(5)
    b = roma_amd.sample_matches(xd, cd, num=NUM, sample_thresh=THRESH, return_indices=True)[2]
    assert torch.equal(a, b) and not torch.equal(a, roma_amd.sample_matches(xd, cd, num=NUM, sample_thresh=THRESH, return_indices=True)[2])
    same = roma_amd.sample_matches(torch.stack([xd[0], xd[0]]), torch.stack([cd[0], cd[0]]), num=NUM, sample_thresh=THRESH, seed=7,
                                   return_indices=True)[2]
    assert torch.equal(same[0], same[1])  # an int seeds every pair alike
    with pytest.raises(ValueError, match="not batched"):
        roma_amd.sample_matches(torch.zeros(1, 70000, 4, device=DEV), torch.ones(1, 70000, device=DEV), num=17000)


def test_chain_into_batched_homography():
    """sample_batched on a synthetic dense warp of a known homography -> to_pixel_coordinates -> find_homography(counts=counts);
    the second pair has fewer certain pixels than num, so its tail is filler that counts must keep out of the fit"""
    import roma_amd
    from roma_amd.matcher import RegressionMatcher
    Hh, Ww, size, num = 48, 48, 480, 1000
    Hs = np.array([[[1.05, 0.03, 12.0], [-0.02, 0.98, -7.0], [2e-5, -1e-5, 1.0]],
                   [[0.93, -0.06, 30.0], [0.05, 1.02, 9.0], [-3e-5, 2e-5, 1.0]]])
    g = (np.arange(Hh) + 0.5) / Hh * 2 - 1
    xa = np.stack(np.meshgrid(g, g, indexing="xy"), -1)                       # [H, W, 2] normalised (x, y) of image A
    warp, cert = np.zeros((2, Hh, Ww, 4), np.float32), np.zeros((2, Hh, Ww), np.float32)
    for b in range(2):
        pa = np.concatenate([size / 2 * (xa + 1), np.ones((Hh, Ww, 1))], -1) @ Hs[b].T
        xb = pa[..., :2] / pa[..., 2:] * 2 / size - 1
        warp[b] = np.concatenate([xa, xb], -1)
        cert[b] = (np.abs(xb).max(-1) < 1) * 0.9
    cert[1, 12:] = 0                                                          # 12 rows of 48: at most 576 certain pixels
    m = RegressionMatcher.__new__(RegressionMatcher)
    m.sample_mode, m.sample_thresh = "threshold_balanced", THRESH
    sm, sc, counts = m.sample_batched(torch.as_tensor(warp).to(DEV), torch.as_tensor(cert).to(DEV), num=num, seed=3, return_counts=True)
    kA, kB = m.to_pixel_coordinates(sm, size, size, size, size)
    assert kA.shape == (2, num, 2) and kB.shape == (2, num, 2)
    npos = [int((cert[b] > 0).sum()) for b in range(2)]
    assert npos[0] >= num and npos[1] < num and counts.tolist() == [num, npos[1]]
    Hd, mask, ok = roma_amd.find_homography(kA, kB, ransac_reproj_threshold=1.0, seed=1, counts=counts)
    torch.cuda.synchronize()
    assert ok.tolist() == [True, True]
    for b in range(2):
        err = corner_error(Hd[b].cpu().numpy(), Hs[b], size)
        print(f"pair {b}: corner error {err:.2e} px, {int(mask[b].sum())} inliers of {int(counts[b])}")
        assert err < 1.0 and int(mask[b].sum()) > 0.9 * int(counts[b]) and not bool(mask[b, int(counts[b]):].any())
