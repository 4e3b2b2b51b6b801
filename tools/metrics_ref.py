"""numpy float64 restatement of the benchmark scoring kernels (csrc/metrics.hip; the definition is in include/roma_hip.h): the
oracle of tests/test_gpu_metrics.py, held to the recorded outputs of the unmodified reference by tests/test_cpu_metrics.py.

Every expression is written out as scalar float64 operations in the order the device evaluates them (Python floats round each
operation once and fuse nothing), so that for equal inputs the arguments of `acos` are bit-equal on both sides and everything
without a transcendental is expected to agree bit for bit.

  pose_error           romatch/utils/utils.py:115-132 (angle_error_mat, angle_error_vec, compute_pose_error) with the benchmarks'
                       e_pose = max(e_t, e_R) and 90-degree fallback (megadepth_pose_estimation_benchmark.py:85-94,
                       scannet_benchmark.py:113-119)
  corner_error         hpatches_sequences_homog_benchmark.py:89-104 (the fallback matrix, lines 89-91; the distance, lines 92-103)
  summary              the closed form of pose_auc (utils.py:135-147) and the accuracy lines
                       (megadepth_pose_estimation_benchmark.py:99-116, scannet_benchmark.py:126-143), reduced in the device's order
  pose_auc_sorted      pose_auc as the reference computes it - sort, prepend the origin, trapezoid - written out: the second
                       route the closed form is checked against
"""
import math

import numpy as np

RAD2DEG = 180.0 / math.pi  # numpy's rad2deg multiplies by this double
THREADS, WAVE = 256, 64
NAN = float("nan")


def _clip1(c):
    return -1.0 if c < -1.0 else (1.0 if c > 1.0 else c)  # a NaN stays, as in np.clip


def pose_cosines(R, t, T_gt):
    """the two clipped cosines of one pair - the arguments the device hands to acos"""
    r = [float(x) for x in np.asarray(R, dtype=np.float64).reshape(9)]
    t0, t1, t2 = (float(x) for x in np.asarray(t, dtype=np.float64).reshape(3))
    T = np.asarray(T_gt, dtype=np.float64)
    g = [float(T[i, j]) for i in range(3) for j in range(3)]
    g0, g1, g2 = float(T[0, 3]), float(T[1, 3]), float(T[2, 3])
    n = math.sqrt((t0 * t0 + t1 * t1) + t2 * t2) * math.sqrt((g0 * g0 + g1 * g1) + g2 * g2)
    ct = _clip1(_div((t0 * g0 + t1 * g1) + t2 * g2, n))
    tr = r[0] * g[0]
    for q in range(1, 9):
        tr = tr + r[q] * g[q]
    cr = _clip1((tr - 1.0) / 2.0)
    return ct, cr


def _acos(c):
    return NAN if c != c else math.acos(c)


def pose_angles(R, t, T_gt):
    """the two angles of one pair in degrees as they come from acos, before e_t is folded into [0, 90]: the folding subtracts from
    180 exactly, so a difference between two acos implementations reaches e_t in ulps of THIS angle, not of the folded one"""
    ct, cr = pose_cosines(R, t, T_gt)
    return _acos(ct) * RAD2DEG, abs(_acos(cr)) * RAD2DEG


def pose_error(R, t, T_gt, ok=True):
    """(e_t, e_R, e_pose) in degrees of one pair"""
    if not ok:
        return 90.0, 90.0, 90.0
    ct, cr = pose_cosines(R, t, T_gt)
    a = _acos(ct) * RAD2DEG
    f = 180.0 - a
    e_t = f if f < a else a
    e_R = abs(_acos(cr)) * RAD2DEG
    return e_t, e_R, (e_R if e_R > e_t else e_t)


def pose_errors(R, t, T_gt, ok=None):
    """the batch: float64 [B, 3]"""
    B = len(R)
    t = np.asarray(t, dtype=np.float64).reshape(B, 3)
    return np.array([pose_error(R[b], t[b], T_gt[b], True if ok is None else bool(ok[b])) for b in range(B)], dtype=np.float64).reshape(B, 3)


def _div(a, b):
    """IEEE division of Python floats (Python raises where the device gives inf or NaN)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _through(h, x, y):
    X = (h[0] * x + h[1] * y) + h[2]
    Y = (h[3] * x + h[4] * y) + h[5]
    Z = (h[6] * x + h[7] * y) + h[8]
    return _div(X, Z), _div(Y, Z)


FALLBACK_H = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)  # hpatches_sequences_homog_benchmark.py:89-91


def corner_error(H_pred, H_gt, sizes, ok=True):
    """the HPatches corner distance of one pair; sizes = (w1, h1, w2, h2)"""
    hp = [float(x) for x in np.asarray(H_pred, dtype=np.float64).reshape(9)] if ok else list(FALLBACK_H)
    hg = [float(x) for x in np.asarray(H_gt, dtype=np.float64).reshape(9)]
    w1, h1, w2, h2 = (float(x) for x in sizes)
    xe, ye = w1 - 1.0, h1 - 1.0
    total = 0.0
    for x, y in ((0.0, 0.0), (0.0, ye), (xe, 0.0), (xe, ye)):
        rx, ry = _through(hg, x, y)
        px, py = _through(hp, x, y)
        dx, dy = rx - px, ry - py
        total = total + math.sqrt(dx * dx + dy * dy)
    side = w2 if w2 < h2 else h2
    return _div(total / 4.0, side / 480.0)


def corner_errors(H_pred, H_gt, sizes, ok=None):
    return np.array([corner_error(H_pred[b], H_gt[b], sizes[b], True if ok is None else bool(ok[b])) for b in range(len(H_pred))],
                    dtype=np.float64)


def summary(errors, thresholds):
    """roma_op_error_summary: dict n, below [T] (int), acc [T], auc [T], and the reduced L, S, M per threshold - reduced as the one
    workgroup does: thread j takes the errors j, j + 256, ... in ascending order, each wave of 64 threads folds by offsets 32 .. 1,
    the four waves are added in order.  The lanes are carried as numpy vectors (elementwise float64 adds, one rounding each);
    a masked-out error adds +0.0, which changes no bit of a sum that is never negative."""
    e = np.asarray(errors, dtype=np.float64).reshape(-1)
    n = e.size
    rounds = -(-n // THREADS)
    pad = np.full(rounds * THREADS, np.inf)
    pad[:n] = e
    pad = pad.reshape(rounds, THREADS)
    out = {"n": n, "below": [], "acc": [], "auc": [], "S": [], "M": []}
    for thr in (float(x) for x in thresholds):
        L = np.zeros(THREADS, dtype=np.int64)
        S = np.zeros(THREADS, dtype=np.float64)
        M = np.zeros(THREADS, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            for r in range(rounds):
                below = pad[r] < thr  # NaN and inf: never
                v = np.where(below, pad[r], 0.0)
                L = L + below
                S = S + v
                M = np.where(v > M, v, M)
        L, S, M = L.reshape(-1, WAVE), S.reshape(-1, WAVE), M.reshape(-1, WAVE)
        off = WAVE // 2
        while off >= 1:
            L[:, :off] = L[:, :off] + L[:, off:2 * off]
            S[:, :off] = S[:, :off] + S[:, off:2 * off]
            M[:, :off] = np.where(M[:, off:2 * off] > M[:, :off], M[:, off:2 * off], M[:, :off])
            off //= 2
        l, s, m = int(L[0, 0]), float(S[0, 0]), float(M[0, 0])
        for w in range(1, THREADS // WAVE):
            l = l + int(L[w, 0])
            s = s + float(S[w, 0])
            m = float(M[w, 0]) if float(M[w, 0]) > m else m
        N = float(n)
        out["below"].append(l)
        out["acc"].append(_div(float(l), N))
        out["auc"].append(_div(((float(l) * thr) - s) + m / 2.0, N * thr))
        out["S"].append(s)
        out["M"].append(m)
    return out


def pose_auc(errors, thresholds):
    """the closed form alone: [T] floats"""
    return summary(errors, thresholds)["auc"]


def pose_auc_sorted(errors, thresholds):
    """utils.py:135-147 written out: the errors sorted (NaN last, as numpy sorts), the origin prepended, recall i / N, the curve cut at
    the first error that is not below the threshold (searchsorted on the left) and closed at the threshold with the last recall, the
    trapezoid rule added left to right, over the threshold.  N = 0 is NaN here as on the device (the reference's empty curve gives
    0)."""
    e = np.sort(np.asarray(errors, dtype=np.float64).reshape(-1))
    n = e.size
    out = []
    for thr in (float(x) for x in thresholds):
        if n == 0:
            out.append(NAN)
            continue
        last = 0
        while last < n and e[last] < thr:
            last += 1
        area, prev_e, prev_r = 0.0, 0.0, 0.0
        for i in range(last):
            cur_e, cur_r = float(e[i]), float(i + 1) / float(n)
            area = area + (cur_e - prev_e) * (cur_r + prev_r) / 2.0
            prev_e, prev_r = cur_e, cur_r
        area = area + (thr - prev_e) * (prev_r + prev_r) / 2.0
        out.append(area / thr)
    return out


def pose_summary(errors):
    """the dict of megadepth_pose_estimation_benchmark.py:99-116 / scannet_benchmark.py:126-143 from the summary at 5, 10, 15, 20"""
    s = summary(errors, (5.0, 10.0, 15.0, 20.0))
    acc, auc = s["acc"], s["auc"]
    return {"auc_5": auc[0], "auc_10": auc[1], "auc_20": auc[3], "map_5": acc[0], "map_10": float(np.mean(acc[:2])),
            "map_20": float(np.mean(acc))}


def homography_summary(errors):
    """hpatches_sequences_homog_benchmark.py:107-113"""
    auc = summary(errors, [float(k) for k in range(1, 11)])["auc"]
    return {"hpatches_homog_auc_3": auc[2], "hpatches_homog_auc_5": auc[4], "hpatches_homog_auc_10": auc[9]}


def hpatches_coordinates(matches, w1, h1, w2, h2):
    """hpatches_sequences_homog_benchmark.py:32-54"""
    m = np.asarray(matches)
    a = np.stack((w1 * (m[..., 0] + 1) / 2, h1 * (m[..., 1] + 1) / 2), axis=-1) - 0.5
    b = np.stack((w2 * (m[..., 2] + 1) / 2, h2 * (m[..., 3] + 1) / 2), axis=-1) - 0.5
    return a, b
