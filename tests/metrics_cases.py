"""The cases shared by tests/test_cpu_metrics.py and tests/test_gpu_metrics.py, generated deterministically, and what
tools/make_metrics_goldens.py records of the unmodified reference on them (tests/golden/metrics_reference.npz).

Pose rows (`pose_cases`, 257 of them so that the device tests reach B = 257; the golden holds the first GOLDEN_POSE_ROWS with the
reference's compute_pose_error on them).  `kind` names each row:
  spread        a random R_gt and t_gt; R = R_gt times a rotation by an angle spread over [1, 179] degrees about a random axis, t = t_gt
                turned by an angle spread over [1, 179] degrees and rescaled
  same_exact    R bit-equal to R_gt, a signed permutation, and t = 2 t_gt with t_gt = (1, 2, 2): both cosines are exactly 1
  same_random   R bit-equal to a random R_gt: the trace is 3 up to rounding, so e_R is 0 or some 1e-6 degrees
  pi            R_gt = I and R = diag(1, -1, -1): the cosine is exactly -1
  antiparallel  t = -t_gt / 2: 180 degrees, which the sign ambiguity folds to 0
  orthogonal    t_gt = (1, 2, 2), t = (2, -1, 0): exactly 90 degrees
  zero_t        t = 0: 0 / 0, e_t and e_pose are NaN
  not_ok        ok == 0 with NaN, inf and 1e300 in R and t: (90, 90, 90)

Error sets (`error_sets`) are made with integer arithmetic only, so every machine generates the same bits and the golden holds
their checksums and the reference's pose_auc on them, not the sets: a 64-bit LCG gives u, the error is (u mod 4096)^2 / 2^16 - a
multiple of 2^-16 below 256, dense near 0 with a long tail, full of ties - and fixed positions are overwritten with 0, 5, 10, 20
(exactly on a threshold), 90 (a failed pair), +inf and NaN."""
import functools
import os
import sys

import numpy as np

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import metrics_ref as mr  # noqa: E402

GOLDEN_FILE = os.path.join(GOLDEN, "metrics_reference.npz")
N_POSE = 257
GOLDEN_POSE_ROWS = 65
BATCHES = (1, 63, 64, 65, 257)
SPECIAL_KINDS = ("same_exact", "same_random", "pi", "antiparallel", "orthogonal", "zero_t", "not_ok", "not_ok")
POSE_THRESHOLDS = (5.0, 10.0, 15.0, 20.0)
REFERENCE_POSE_THRESHOLDS = (5.0, 10.0, 20.0)
HOMOGRAPHY_THRESHOLDS = tuple(float(k) for k in range(1, 11))
SET_SIZES = (0, 1, 2, 255, 256, 257, 7500, 65536)


def _rodrigues(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _perpendicular(v, rng):
    w = np.cross(v, rng.standard_normal(3))
    return w / np.linalg.norm(w)


@functools.lru_cache(maxsize=None)
def pose_cases():
    """dict R f64 [257, 3, 3], t f64 [257, 3], T f64 [257, 3, 4], ok u8 [257], kind (tuple of 257 names); read-only arrays.
    Row 0 is a spread row, rows 1 - 8 the special ones, the rest spread."""
    rng = np.random.default_rng(20)
    n_spread = N_POSE - len(SPECIAL_KINDS)
    ang_R = np.deg2rad(rng.permutation(np.linspace(1.0, 179.0, n_spread)))
    ang_t = np.deg2rad(rng.permutation(np.linspace(1.0, 179.0, n_spread)))
    kinds = ["spread"] + list(SPECIAL_KINDS) + ["spread"] * (n_spread - 1)
    R, t, T, ok = [], [], [], []
    k = 0
    exact_t = np.array([1.0, 2.0, 2.0])
    for kind in kinds:
        Rg = _rodrigues(rng.standard_normal(3), rng.uniform(0.0, np.pi))
        tg = rng.standard_normal(3) * rng.uniform(0.1, 3.0)
        Re, te, good = Rg.copy(), tg.copy(), 1
        if kind == "spread":
            Re = Rg @ _rodrigues(rng.standard_normal(3), ang_R[k])
            te = (_rodrigues(_perpendicular(tg, rng), ang_t[k]) @ tg) * rng.uniform(0.2, 5.0)
            k += 1
        elif kind == "same_exact":
            Rg = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
            Re, tg, te = Rg.copy(), exact_t, 2.0 * exact_t
        elif kind == "pi":
            Rg, Re = np.eye(3), np.diag([1.0, -1.0, -1.0])
        elif kind == "antiparallel":
            tg = exact_t
            te = -tg / 2.0
        elif kind == "orthogonal":
            tg, te = exact_t, np.array([2.0, -1.0, 0.0])
        elif kind == "zero_t":
            te = np.zeros(3)
        elif kind == "not_ok":
            good = 0
            Re = np.array([[np.nan, np.inf, 1e300], [-np.inf, 0.0, 1.0], [np.nan, -1e300, 2.0]])
            te = np.array([np.nan, 0.0, np.inf]) if len(ok) % 2 else np.array([1e300, -1e300, 1e300])
        R.append(Re), t.append(te), T.append(np.concatenate([Rg, tg[:, None]], axis=1)), ok.append(good)
    out = {"R": np.stack(R), "t": np.stack(t), "T": np.stack(T), "ok": np.array(ok, dtype=np.uint8)}
    for a in out.values():
        a.setflags(write=False)
    out["kind"] = tuple(kinds)
    return out


@functools.lru_cache(maxsize=None)
def corner_cases():
    """dict Hp, Hg f64 [257, 3, 3], sizes f64 [257, 4], ok u8 [257], kind.  Row 0 is a random row; then: `same` (H_pred bit-equal to
    H_gt: 0), `shift` (identity against a translation by (3, 4): 5 * 480 / min(w2, h2)), `not_ok` twice (garbage in H_pred, scored
    with the fallback matrix), `zero_row` (third row of H_pred zero: division by zero at every corner), `zero_left` (third
    coordinate x: zero at the two left corners); the rest random"""
    rng = np.random.default_rng(21)
    special = ("same", "shift", "not_ok", "not_ok", "zero_row", "zero_left")
    kinds = ["random"] + list(special) + ["random"] * (N_POSE - 1 - len(special))
    Hp, Hg, sizes, ok = [], [], [], []
    for kind in kinds:
        sz = rng.integers(300, 1601, 4).astype(np.float64)
        G = np.array([[1.0 + 0.1 * rng.standard_normal(), 0.08 * rng.standard_normal(), 30.0 * rng.standard_normal()],
                      [0.08 * rng.standard_normal(), 1.0 + 0.1 * rng.standard_normal(), 30.0 * rng.standard_normal()],
                      [1e-4 * rng.standard_normal(), 1e-4 * rng.standard_normal(), 1.0]])
        P = G + np.array([[1e-2, 1e-2, 3.0], [1e-2, 1e-2, 3.0], [1e-5, 1e-5, 0.0]]) * rng.standard_normal((3, 3)) * rng.uniform(0.0, 2.0)
        good = 1
        if kind == "same":
            P = G.copy()
        elif kind == "shift":
            G, P = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, 4.0], [0.0, 0.0, 1.0]]), np.eye(3)
        elif kind == "not_ok":
            good = 0
            P = np.full((3, 3), np.nan) if len(ok) % 2 else np.array([[np.inf, 1e300, 0.0], [0.0, -np.inf, 0.0], [0.0, 0.0, 0.0]])
        elif kind == "zero_row":
            P[2] = 0.0
        elif kind == "zero_left":
            P[2] = (1.0, 0.0, 0.0)
        Hp.append(P), Hg.append(G), sizes.append(sz), ok.append(good)
    out = {"Hp": np.stack(Hp), "Hg": np.stack(Hg), "sizes": np.stack(sizes), "ok": np.array(ok, dtype=np.uint8)}
    for a in out.values():
        a.setflags(write=False)
    out["kind"] = tuple(kinds)
    return out


def _lcg(n, seed):
    """n values of a 64-bit LCG (Knuth's MMIX constants), its top 32 bits: integer arithmetic, the same on every machine"""
    out = np.empty(n, dtype=np.uint64)
    x = seed
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out[i] = x >> 32
    return out


@functools.lru_cache(maxsize=None)
def error_sets():
    """dict name -> read-only float64 errors: n0 ... n65536 (SET_SIZES) and none_below (300 errors, none below 25)"""
    sets = {}
    for n in SET_SIZES:
        u = _lcg(n, 1000 + n)
        e = ((u % np.uint64(4096)).astype(np.float64) ** 2) / 65536.0
        if n == 1:
            e[:] = [3.0]
        elif n == 2:
            e[:] = [0.0, 5.0]
        elif n >= 255:
            e[3::10] = 90.0  # the failed pairs
            e[7], e[17], e[27], e[37], e[47] = 0.0, 5.0, 10.0, 20.0, 15.0
            e[57], e[67], e[77], e[87] = np.inf, np.nan, e[76], 0.0  # and a tie with the neighbour
            e[n - 1], e[n - 2] = 20.0, np.nan
        sets[f"n{n}"] = e
    u = _lcg(300, 7)
    e = 25.0 + (u % np.uint64(4096)).astype(np.float64) / 64.0
    e[3::10], e[5], e[6] = 90.0, np.inf, np.nan
    sets["none_below"] = e
    for a in sets.values():
        a.setflags(write=False)
    return sets


def checksum(e):
    """order-dependent 64-bit checksum of the bits of a float64 array"""
    bits = np.ascontiguousarray(e, dtype=np.float64).view(np.uint64)
    weights = np.arange(1, bits.size + 1, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return int((bits * weights).sum(dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/metrics_reference.npz: the first GOLDEN_POSE_ROWS pose rows (in_*), the reference's compute_pose_error on those
    with ok == 1 (ref_e_t, ref_e_R; NaN-filled for the others, which the reference never sees), per error set its checksum
    (chk_<name>) and the reference's pose_auc at 5, 10, 20 (ref_auc_pose_<name>) and at 1 .. 10 (ref_auc_homog_<name>)"""
    with np.load(GOLDEN_FILE) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle():
    """tools/metrics_ref.py on all the cases, computed once: pose f64 [257, 3], corner f64 [257], summary {name: {thresholds: dict}}"""
    p, c = pose_cases(), corner_cases()
    out = {"pose": mr.pose_errors(p["R"], p["t"], p["T"], p["ok"]), "corner": mr.corner_errors(c["Hp"], c["Hg"], c["sizes"], c["ok"]),
           "summary": {name: {thr: mr.summary(e, thr) for thr in (POSE_THRESHOLDS, HOMOGRAPHY_THRESHOLDS)}
                       for name, e in error_sets().items()}}
    # one ulp of each pair's angles as acos returns them (e_t before it is folded; e_pose is either): the unit of the device test
    unit = np.full((N_POSE, 3), np.spacing(90.0))
    for b in range(N_POSE):
        if p["ok"][b]:
            a_t, a_R = (np.spacing(a) if a == a else np.spacing(180.0) for a in mr.pose_angles(p["R"][b], p["t"][b], p["T"][b]))
            unit[b] = (a_t, a_R, max(a_t, a_R))
    out["pose_unit"] = unit
    for k in ("pose", "corner", "pose_unit"):
        out[k].setflags(write=False)
    return out


def auc_bound(n):
    """(N + 8) 2^-52: twice the worst-case rounding of an N-term sum, relative"""
    return (n + 8) * 2.0 ** -52
