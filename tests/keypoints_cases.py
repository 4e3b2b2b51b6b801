"""The cases shared by tests/test_cpu_keypoints_batched.py and tests/test_gpu_keypoints_batched.py, built from the committed goldens
tests/golden/keypoints_reference.npz and keypoints_ties_reference.npz (the reference's own match_keypoints on a seeded warp).

  BATCH     seven pairs padded to NA = 700, NB = 900:
              0  the keypoints golden in full (700 x 900)          4  na = 0
              1  the ties golden in full (360 x 517)               5  nb = 0
              2  keypoints-golden prefixes 257 x 511               6  the keypoints golden on the vertically flipped warp and
              3  prefixes 256 x 512                                   certainty
            sizes on and one off the workgroup of 256 rows; pair 1 has duplicate keypoints, so more pairs than distinct rows;
  GENERATED one pair of 1300 x 2100 points on the golden's warp, past the LDS tile of 1024 and the slice split in both directions:
            from np.random.default_rng(5), 900 points of B are p_i + 0.002 N(0, 1), 1000 are uniform, 200 exact duplicates (of the
            first 200 points) are appended and the set is permuted: 1068 pairs on 874 distinct rows of A;
  TIES_MATCHED  the ties golden with only the matched rows of A: more pairs than rows of A, for the cap on max_matches;
  PARAMS    the two parameter sets of the goldens.

Every case is checked here, on the CPU, before a device test sees it: the smallest relative gap between a row's or column's minimum
and the next distinct distance is at least MIN_GAP (far above float32 rounding, so no arithmetic can pick another pair; equal bits
from duplicate points tie in any arithmetic and are no gap), and the numpy restatement tools/keypoints_ref.py returns exactly the
pairs of oracle.match_keypoints (torch cdist + nonzero).  A device mismatch can then never be explained by a near-tie."""
import functools
import os
import sys

import numpy as np
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import keypoints_ref as kr  # noqa: E402

PARAMS = {"default": {}, "loose": dict(max_dist=0.02, cert_th=0.6)}
NA, NB = 700, 900
MIN_GAP = 1e-5
# pairs per case and parameter set: the goldens' own lengths, and what restatement and oracle both give for the derived cases
PAIRS = {0: {"default": 478, "loose": 420}, 1: {"default": 349, "loose": 278}, 2: {"default": 132, "loose": 128},
         "generated": {"default": 1068, "loose": 882}}


@functools.lru_cache(maxsize=None)
def golden(name):
    """'keypoints' or 'keypoints_ties': warp [96, 128, 4], cert, x_A, x_B and inds_{A,B}_{default,loose}, read-only"""
    with np.load(os.path.join(GOLDEN, f"{name}_reference.npz")) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


def golden_inds(name, params):
    g = golden(name)
    return np.stack([g["inds_A_" + params], g["inds_B_" + params]], axis=-1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def pairs():
    """the seven pairs as (x_a [na, 2], x_b [nb, 2], warp, cert), unpadded"""
    k, t = golden("keypoints"), golden("keypoints_ties")
    flip_w, flip_c = np.ascontiguousarray(k["warp"][::-1]), np.ascontiguousarray(k["cert"][::-1])
    return ((k["x_A"], k["x_B"], k["warp"], k["cert"]),
            (t["x_A"], t["x_B"], t["warp"], t["cert"]),
            (k["x_A"][:257], k["x_B"][:511], k["warp"], k["cert"]),
            (k["x_A"][:256], k["x_B"][:512], k["warp"], k["cert"]),
            (k["x_A"][:0], k["x_B"][:333], k["warp"], k["cert"]),
            (k["x_A"][:300], k["x_B"][:0], k["warp"], k["cert"]),
            (k["x_A"], k["x_B"], flip_w, flip_c))


@functools.lru_cache(maxsize=None)
def ties_matched():
    """the ties golden with only those rows of A that have a match: duplicate keypoints of B then give MORE pairs than A has rows"""
    t = golden("keypoints_ties")
    rows = np.unique(np.concatenate([t["inds_A_default"], t["inds_A_loose"]]))
    return np.ascontiguousarray(t["x_A"][rows]), t["x_B"], t["warp"], t["cert"]


def case_data(case):
    """(x_a, x_b, warp, cert) of a pair number of the batch, 'generated' or 'ties_matched'"""
    return generated() if case == "generated" else ties_matched() if case == "ties_matched" else pairs()[case]


def pad(rows, width, fill=0.0):
    out = np.full((width, 2), fill, dtype=np.float32)
    out[:len(rows)] = rows
    return out


def batch(order=None, na_pad=NA, nb_pad=NB, fill=0.0):
    """the pairs `order` (default all seven) as one padded batch of numpy arrays; the padding rows hold `fill`"""
    ps = [case_data(i) for i in (range(len(pairs())) if order is None else order)]
    return dict(x_A=np.stack([pad(p[0], na_pad, fill) for p in ps]), x_B=np.stack([pad(p[1], nb_pad, fill) for p in ps]),
                counts_A=np.array([len(p[0]) for p in ps], np.int32), counts_B=np.array([len(p[1]) for p in ps], np.int32),
                warp=np.stack([p[2] for p in ps]), cert=np.stack([p[3] for p in ps]))


@functools.lru_cache(maxsize=None)
def generated():
    """(x_a [1300, 2], x_b [2100, 2], warp, cert)"""
    g = golden("keypoints")
    rng = np.random.default_rng(5)
    x_a = (rng.random((1300, 2)) * 1.9 - 0.95).astype(np.float32)
    p, _ = kr.sample_warp_at(g["warp"], g["cert"], x_a)
    near = p[:900] + (0.002 * rng.standard_normal((900, 2))).astype(np.float32)
    x_b = np.concatenate([near, (rng.random((1000, 2)) * 2 - 1).astype(np.float32)]).astype(np.float32)
    x_b = np.concatenate([x_b, x_b[:200]])
    x_b = x_b[rng.permutation(len(x_b))]
    return x_a, x_b, g["warp"], g["cert"]


def oracle_inds(x_a, x_b, warp, cert, **kw):
    """oracle.match_keypoints (torch grid_sample + cdist + nonzero on the CPU) as [n, 2] int64"""
    from oracle import roma_oracle as O
    if len(x_a) == 0 or len(x_b) == 0:
        return np.zeros((0, 2), np.int64)
    i, j = O.match_keypoints(*(torch.from_numpy(np.array(a)) for a in (x_a, x_b, warp, cert)), **kw)
    return np.stack([i.numpy(), j.numpy()], axis=-1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def checked(case, params):
    """the restatement's pairs [n, 2] int64 of `case` (a pair number of the batch, 'generated' or 'ties_matched') after the two checks above;
    also (gap, p, c) for the tests that report or compare them"""
    x_a, x_b, warp, cert = case_data(case)
    inds, p, c, d2 = kr.match_pair(x_a, x_b, warp, cert, **PARAMS[params])
    gap = kr.min_gap(d2)
    assert gap >= MIN_GAP, (case, params, gap)
    ref = oracle_inds(x_a, x_b, warp, cert, **PARAMS[params])
    assert np.array_equal(inds, ref), (case, params, len(inds), len(ref))
    inds.setflags(write=False)
    return inds, gap, p, c


def expected(case, params):
    return checked(case, params)[0]
