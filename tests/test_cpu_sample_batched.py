"""tools/sample_ref.py (the oracle of roma_amd.sample_matches / RegressionMatcher.sample_batched) on the scenes the GPU test runs,
the conditions that test puts on its seeds, and the C ABI of roma_op_sample_matches (dlopen only).  No GPU."""
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
import sample_ref as sr  # noqa: E402

NEW_SYMBOLS = ("roma_op_sample_matches", "roma_op_sample_matches_workspace")
N, NUM, K, M = 4000, 500, 2000, 500  # rows per pair, num, first draw (4 num), result: K is a multiple of neither 256 nor 1024
THRESH = 0.05
MODES = ("threshold_balanced", "threshold", "balanced", "plain")
# one seed per pair, found by a search over 0, 1, 2, ... for the conditions test_seeds_keep_the_cut_clear_of_rounding asserts
# (pair 1 also: a tie AT the cut of the first draw).  The GPU test asserts the same conditions again on what it compares.
SEEDS = (0, 9699, 200, 300)
GAP = 1e-4       # relative gap the GPU test needs between the last key taken and the next distinct one (__logf: ~1e-6)
GAP_CPU = 2e-4   # what the seeds hold here for the first draw (float64 keys, the ones the GPU test compares against)
GAP_CPU2 = 5e-4  # and for the second draw, which is driven by the float64 density here and by the device's (1e-5 off) there


@functools.lru_cache(maxsize=None)
def two_clusters():
    """the scene of test_gpu_ops.test_sample_distribution_matches_oracle: (matches [4000, 4], certainty [4000]) float32"""
    gen = torch.Generator().manual_seed(3)
    dense = torch.tensor([0.3, -0.2, 0.1, 0.4]) + 0.02 * torch.randn(3000, 4, generator=gen)
    loose = torch.tensor([-0.5, 0.5, -0.4, -0.3]) + 0.08 * torch.randn(1000, 4, generator=gen)
    cert = torch.full((4000,), 0.5)
    cert[:10] = 0.01
    return torch.cat([dense, loose]).numpy(), cert.numpy()


@functools.lru_cache(maxsize=None)
def pairs():
    """(matches [4, N, 4], certainty [4, N]) float32:
    0 the two clusters, certainties 0.5 and ten of 0.01; 1 every certainty above the threshold (all weights 1: tied keys);
    2 only 1 500 positive certainties (filler rows in the first draw); 3 only 300 (filler rows in the result: counts = 300)"""
    rng = np.random.default_rng(7)
    x0, c0 = two_clusters()
    x = np.stack([x0, rng.uniform(-1, 1, (N, 4)).astype(np.float32), x0[rng.permutation(N)], x0[rng.permutation(N)]])
    c = np.zeros((4, N), dtype=np.float32)
    c[0] = c0
    c[1] = 0.9
    for b, npos in ((2, 1500), (3, 300)):
        pos = rng.choice(N, npos, replace=False)
        c[b, pos] = np.where(rng.random(npos) < 0.7, 0.8, 0.02).astype(np.float32)
    return x, c


def cut_gaps(keys, k):
    """(relative gap from the k-th smallest key T to the next larger one, relative gap from the next smaller one to T if the
    entries equal to T are only partly taken else inf, number of entries equal to T, how many of them are taken).  A +inf T has
    no larger key and, all +inf keys being equal, an exact tie rule: both gaps inf."""
    s = np.sort(keys)
    T = s[k - 1]
    ties, taken = int((s == T).sum()), int((s[:k] == T).sum())
    if np.isinf(T):
        return np.inf, np.inf, ties, taken
    above = s[s > T]
    up = np.inf if len(above) == 0 or np.isinf(above[0]) else (above[0] - T) / T
    below = s[s < T]
    down = (T - below[-1]) / T if taken < ties and len(below) else np.inf
    return float(up), float(down), ties, taken


def ascending(keys, tol=1e-5):
    """keys in draw order: non-decreasing to `tol` relative (+inf behind everything)"""
    a, b = keys[:-1], keys[1:]
    with np.errstate(invalid="ignore"):
        return bool(np.all((b >= a * (1 - tol)) | (np.isinf(a) & np.isinf(b))))


def oracle(b, mode="threshold_balanced", n=N, num=NUM, seed=None):
    x, c = pairs()
    return sr.sample(x[b, :n], c[b, :n], num, mode, THRESH, SEEDS[b] if seed is None else seed)


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_uniforms_are_the_devices_integers():
    """mix64 against Python integers, and u = (23 bits + 0.5) / 2^23 inside (0, 1)"""
    def mix(z):
        z &= sr.MASK
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & sr.MASK
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & sr.MASK
        return z ^ (z >> 31)
    for seed in (0, 1, 12345678901234567, 2 ** 62 - 1, 2 ** 64 - 1):
        u = sr.uniforms(seed, 50)
        for i in (0, 1, 7, 49):
            r = mix(mix(seed + 0x9e3779b97f4a7c15 * (i + 1)) ^ seed)
            assert u[i] == ((r >> 41) + 0.5) / 8388608.0
        assert np.all((u > 0) & (u < 1)) and np.all(u * 8388608.0 - 0.5 == np.round(u * 8388608.0 - 0.5))
    assert sr.SECOND_DRAW_SEED == 0x5851f42d4c957f2d
    source = open(os.path.join(ROOT, "roma_amd", "csrc", "sample_batched.hip")).read()
    assert "SAMPLE_SECOND_DRAW_SEED = 0x5851f42d4c957f2dull" in source


def test_tie_rule_draw_order_and_filler():
    w = np.array([0, 1, 1, 0, 0, 1, 0], dtype=np.float32)
    for seed in range(20):
        idx, keys = sr.draw(w, 5, seed)
        assert set(idx[:3]) == {1, 2, 5} and list(idx[3:]) == [0, 3]      # the filler: lowest zero-weight indices, in index order
        assert ascending(keys[idx]) and np.all(np.diff(keys[idx[:3]]) >= 0)
    # equal keys: the lower index first and, at the cut, alone
    keys = np.array([2.0, 1.0, 2.0, 3.0, 2.0])
    order = np.lexsort((np.arange(5), keys))
    assert list(order) == [1, 0, 2, 4, 3] and cut_gaps(keys, 2) == (0.5, 0.5, 3, 1) and cut_gaps(keys, 4)[1] == np.inf


def test_p_rule():
    p = sr.balance_weights(np.array([0.0, 9.99, 10.0, 99.0, 99.0]), np.array([1.0, 1.0, 1.0, 0.5, 0.0]))
    assert p.dtype == np.float32 and list(p) == [np.float32(1e-7), np.float32(1e-7), np.float32(1) / np.float32(11), np.float32(0.01), 0]


@pytest.mark.parametrize("mode", MODES)
def test_reference_properties(mode):
    """distinct indices, never a zero-certainty row while positive ones remain, counts, shapes, certainties clipped or not"""
    x, c = pairs()
    for b in range(4):
        o = oracle(b, mode)
        k = K if "balanced" in mode else NUM
        assert o["matches"].shape == (M, 4) and o["certainty"].shape == (M,) and o["first_idx"].shape == (k,)
        assert len(set(o["idx"])) == M and len(set(o["first_idx"])) == k
        npos = int((c[b] > 0).sum())
        assert o["count"] == min(M, npos)
        assert np.all(c[b, o["idx"][:o["count"]]] > 0) and np.all(c[b, o["idx"][o["count"]:]] == 0)
        assert np.all(c[b, o["first_idx"][:min(k, npos)]] > 0) and np.all(c[b, o["first_idx"][min(k, npos):]] == 0)
        if npos < k:  # the filler: the LOWEST zero-certainty indices, in index order
            assert np.array_equal(o["first_idx"][npos:], np.nonzero(c[b] == 0)[0][:k - npos])
        assert np.array_equal(o["matches"], x[b, o["idx"]])
        want = np.where(c[b] > THRESH, np.float32(1), c[b]) if "threshold" in mode else c[b]
        assert np.array_equal(o["certainty"], want[o["idx"]])
        if "balanced" in mode:
            assert ascending(o["keys2"][o["second"]]) and np.array_equal(o["idx"], o["first_idx"][o["second"]])
        assert ascending(o["keys1"][o["first_idx"]])
    o = sr.sample(x[0, :600], c[0, :600], NUM, "threshold_balanced", THRESH, 5)       # k = n
    assert sorted(o["first_idx"]) == list(range(600)) and len(set(o["idx"])) == 500
    dens = np.full(K, 50.0)                                                            # density= drives the second draw
    o2 = sr.sample(x[0], c[0], NUM, "threshold_balanced", THRESH, SEEDS[0], density=dens)
    assert np.array_equal(o2["first_idx"], oracle(0)["first_idx"]) and np.all(o2["p"] == np.float32(1) / np.float32(51))
    assert np.array_equal(o2["second"], sr.draw(o2["p"], M, SEEDS[0] ^ sr.SECOND_DRAW_SEED)[0])


def test_distribution_matches_the_torch_oracle():
    """the statistic, tolerance and number of draws of test_gpu_ops.test_sample_distribution_matches_oracle"""
    from oracle import roma_oracle as O
    x, c = two_clusters()
    fr = [float((sr.sample(x, c, 500, "threshold_balanced", THRESH, seed)["matches"][:, 0] < -0.1).mean()) for seed in (11, 12, 13, 14)]
    gen = torch.Generator().manual_seed(3)
    fo = []
    for _ in range(4):
        om, _ = O.sample(torch.from_numpy(x), torch.from_numpy(c), num=500, generator=gen)
        fo.append(float((om[:, 0] < -0.1).float().mean()))
    assert abs(np.mean(fr) - np.mean(fo)) < 0.08, (fr, fo)
    assert np.mean(fr) > 0.5


def test_seeds_keep_the_cut_clear_of_rounding():
    """what the GPU test relies on, checked here first: at every cut it compares as a set, the next distinct key lies more than
    GAP_CPU away; pair 1 holds tied keys, one tie exactly at the cut of the first draw with only its lower index taken"""
    for b in range(4):
        for mode in MODES:
            o = oracle(b, mode)
            up, down, ties, taken = cut_gaps(o["keys1"], len(o["first_idx"]))
            assert up > GAP_CPU and down > GAP_CPU, (b, mode, up, down)
            if mode == "threshold_balanced":
                up, down, _, _ = cut_gaps(o["keys2"], M)
                assert up > GAP_CPU2 and down > GAP_CPU2, (b, "second", up, down)
                if b == 1:
                    finite = o["keys1"][np.isfinite(o["keys1"])]
                    assert len(np.unique(finite)) < len(finite)
                    assert (ties, taken) == (2, 1)
                    tied = np.nonzero(o["keys1"] == np.sort(o["keys1"])[K - 1])[0]
                    assert tied[0] in o["first_idx"] and tied[1] not in o["first_idx"]
    o = sr.sample(pairs()[0][0, :600], pairs()[1][0, :600], NUM, "threshold_balanced", THRESH, SEEDS[0])
    assert min(cut_gaps(o["keys2"], M)[:2]) > GAP_CPU2


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert len(_lib.SIGNATURES["roma_op_sample_matches"][1]) == 18
    assert len(_lib.SIGNATURES["roma_op_sample_matches_workspace"][1]) == 4
    ws = built_lib.roma_op_sample_matches_workspace
    for bal in (0, 1):
        assert 0 < ws(1, N, NUM, bal) < ws(2, N, NUM, bal) < ws(8, N, NUM, bal)
        assert ws(0, N, NUM, bal) == 0 and ws(-1, N, NUM, bal) == 0 and ws(4, 0, NUM, bal) == 0 and ws(4, N, 0, bal) == 0
        assert ws(4, N, -5, bal) == 0
    assert ws(2, N, NUM, 1) > ws(2, N, NUM, 0)
    assert ws(8, 864 * 1728, 10000, 1) < 1 << 28  # the flagship size: 68 MB


def test_arguments_are_validated_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null 16-byte aligned address: validation must fail before it is used

    def call(*, x=p, c=p, seeds=p, B=2, n=N, num=NUM, bal=1, om=p, oc=p, ws=p, nws=1 << 30):
        return lib.roma_op_sample_matches(x, c, seeds, B, n, num, 1, THRESH, bal, om, oc, None, None, None, None, ws, nws, None)
    for kw, word in ((dict(x=None), b"null"), (dict(c=None), b"null"), (dict(seeds=None), b"null"), (dict(om=None), b"null"),
                     (dict(oc=None), b"null"), (dict(ws=None), b"null"), (dict(B=-1), b"B"), (dict(B=70000), b"B"),
                     (dict(n=-3), b"negative"), (dict(num=-1), b"negative"), (dict(n=1 << 31), b"2^31"),
                     (dict(n=100000, num=16385), b"65536"), (dict(n=100000, num=65537, bal=0), b"65536"),
                     (dict(nws=16), b"workspace"), (dict(nws=-5), b"workspace"), (dict(x=8), b"aligned"), (dict(om=4), b"aligned")):
        assert call(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    assert call(n=100000, num=16385) != 0 and b"not batched" in lib.roma_last_error()  # the message says what the limit is
    assert call(n=100000, num=16384, nws=16) != 0 and b"workspace" in lib.roma_last_error()  # k = 65 536 itself is accepted
    for kw in (dict(B=0), dict(n=0), dict(num=0)):
        assert call(nws=0, **kw) == 0  # nothing to do, nothing launched


def test_python_front_end_refuses_host_tensors_and_large_draws():
    import roma_amd
    from roma_amd import _lib
    from roma_amd.matcher import RegressionMatcher
    assert "sample_matches" in roma_amd.__all__ and callable(RegressionMatcher.sample_batched)
    x, c = torch.zeros(2, 100, 4), torch.ones(2, 100)
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.sample_matches(x, c, num=10)
    m = RegressionMatcher.__new__(RegressionMatcher)
    m.sample_mode, m.sample_thresh = "threshold_balanced", 0.05
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        m.sample_batched(x, c, num=10)


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_sample_batched_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "sample_batched.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/sample_batched.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == sorted(f"sample_{s}_kernel" for s in ("init", "keys", "hist", "scan", "tie_count", "tie_cut", "compact",
                                                           "order_gather", "kde", "density_keys")), names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
