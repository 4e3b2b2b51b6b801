"""Scoring of the pose and homography benchmarks on the device (`roma_op_pose_error`, `roma_op_corner_error`,
`roma_op_error_log_append`, `roma_op_error_summary`, csrc/metrics.hip): the reference's `compute_pose_error` and `pose_auc`
(romatch/utils/utils.py), the accuracy / mAP lines of its MegaDepth and ScanNet pose benchmarks and the corner distance of its
HPatches benchmark.  With them the chain sample_batched -> to_pixel_coordinates -> estimate_pose / find_homography is scored
without reading R, t, ok back: each batch appends its errors to an `ErrorLog` on the device and the only host read is the
summary at the end.  The definition is stated in include/roma_hip.h and restated in numpy float64 by tools/metrics_ref.py.

Conventions are those of `roma_amd.gt_warp`: device tensors (the small ground-truth matrices may also be numpy), every check
runs before anything touches the device, no call synchronises with the host except `ErrorLog.pose_summary` and
`ErrorLog.homography_summary`.  All arithmetic is float64 in a fixed order, so every output is bit-identical from run to run.

The pose loop of the MegaDepth / ScanNet benchmarks (one pair, its five repeats as a batch with five seeds and the pair's
threshold - `estimate_pose` takes one norm_thresh per call):

    log = roma_amd.ErrorLog()
    for pair in pairs:
        ...                                               # match(), sample_batched(), to_pixel_coordinates(): see sample_batched
        R, t, mask, ok = roma_amd.estimate_pose(kpts_A, kpts_B, K1, K2, norm_thresh, seed=seeds)    # [5, N, 2]
        err = roma_amd.pose_error(R, t, T_1to2, ok=ok, log=log)                                      # T_1to2 [5, 3, 4]
        # log.append(err.e_pose[-1:])                     # ScanNet only: its loop appends the last repeat once more
    print(log.pose_summary())                             # the one host read: auc_5 / 10 / 20, map_5 / 10 / 20

and the HPatches loop:

    log = roma_amd.ErrorLog()
    for pair in pairs:
        kpts_A, kpts_B = roma_amd.hpatches_coordinates(matches, w1, h1, w2, h2)
        H, mask, ok = roma_amd.find_homography(kpts_A, kpts_B, 3 * min(w2, h2) / 480, confidence=0.99999)
        roma_amd.homography_corner_error(H, H_gt, (w1, h1, w2, h2), ok=ok, log=log)
    print(log.homography_summary())                       # hpatches_homog_auc_3 / 5 / 10
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream

PoseError = namedtuple("PoseError", "e_t e_R e_pose")
ErrorSummary = namedtuple("ErrorSummary", "n dropped below acc auc")

MAX_BATCH = 65535      # rows of one call (csrc/metrics.hip MT_MAX_B)
MAX_ERRORS = 65536     # errors of one summary, and so the largest log
MAX_THRESHOLDS = 16
POSE_THRESHOLDS = (5.0, 10.0, 15.0, 20.0)
HOMOGRAPHY_THRESHOLDS = tuple(float(k) for k in range(1, 11))


def _device_f64(x, name, shapes, allow_host):
    """shape and type check of one input, nothing touched: returns (x, batched).  shapes: the unbatched shapes allowed"""
    if not isinstance(x, torch.Tensor):
        if not allow_host:
            raise TypeError(f"roma_amd.metrics: {name} must be a torch tensor, got {type(x).__name__}")
        x = np.asarray(x, dtype=np.float64)
    elif not x.dtype.is_floating_point:
        raise ValueError(f"roma_amd.metrics: {name} must be a floating-point tensor, got {x.dtype}")
    shape = tuple(x.shape)
    if shape in shapes:
        return x, False
    if len(shape) >= 1 and shape[1:] in shapes:
        return x, True
    want = " or ".join(f"[B, {', '.join(map(str, s))}]" for s in shapes)
    raise ValueError(f"roma_amd.metrics: {name} must be {want} (or the same without B), got {shape}")


def _upload(x, name, dev, shape):
    """contiguous float64 [*shape] on dev: a device tensor as it is, host numpy uploaded (no synchronisation)"""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise _lib.RomaHipError(f"roma_amd.metrics: {name} must be a tensor on a HIP device; there is no CPU fallback")
        return x.detach().to(device=dev, dtype=torch.float64).reshape(shape).contiguous()
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C").reshape(shape)).to(dev)


def _estimate(x, name):
    """the estimates (R, t, H, values to append) have no host form: they come from the device"""
    if not x.is_cuda:
        raise _lib.RomaHipError(f"roma_amd.metrics: {name} must be a tensor on a HIP device; there is no CPU fallback")
    return x.detach()


def _ok_shape(ok, B, batched):
    if ok is None:
        return
    if not isinstance(ok, torch.Tensor) or ok.dtype not in (torch.bool, torch.uint8):
        raise ValueError("roma_amd.metrics: ok must be a bool or uint8 tensor")
    if tuple(ok.shape) != ((B,) if batched else ()) and not (not batched and tuple(ok.shape) == (1,)):
        raise ValueError(f"roma_amd.metrics: ok must be [{B}], got {tuple(ok.shape)}")


def _ok_bytes(ok, B, dev):
    """ok as uint8 [B] on dev; a bool tensor is reinterpreted, not converted: no launch"""
    if ok is None:
        return None
    ok = _estimate(ok, "ok").to(device=dev).reshape(B).contiguous()
    return ok.view(torch.uint8) if ok.dtype == torch.bool else ok


def _log_check(log):
    if log is not None and not isinstance(log, ErrorLog):
        raise TypeError(f"roma_amd.metrics: log must be an ErrorLog, got {type(log).__name__}")


def _batch_check(B, what):
    if B > MAX_BATCH:
        raise ValueError(f"roma_amd.metrics: {B} {what} is more than one call takes (B <= {MAX_BATCH})")


def _log_args(log, dev):
    if log is None:
        return C.c_void_p(0), 0, C.c_void_p(0)
    if log.device != dev:
        raise ValueError(f"roma_amd.metrics: the ErrorLog lives on {log.device}, the errors on {dev}")
    return _ptr(log._rows), log.capacity, _ptr(log._state)


def pose_error(R, t, T_gt, ok=None, log=None):
    """The reference's `compute_pose_error` for a batch on the device (`roma_op_pose_error`), with the benchmarks' `e_pose =
    max(e_t, e_R)` and their 90-degree fallback.  R [B, 3, 3] and t [B, 3] or [B, 3, 1] as `estimate_pose` returns them (device
    tensors); T_gt [B, 3, 4] or [B, 4, 4], a device tensor or numpy; ok bool [B] (`estimate_pose`'s): a pair with ok False gets
    (90, 90, 90) whatever R and t hold.  log: an `ErrorLog` that e_pose is appended to in the same launch.

    Returns PoseError(e_t, e_R, e_pose), each float64 [B] in degrees (0-dim for the unbatched form R [3, 3]).  e_t is NaN for a
    translation of zero norm, as in the reference."""
    _log_check(log)
    if not isinstance(R, torch.Tensor) or not isinstance(t, torch.Tensor):
        raise TypeError("roma_amd.metrics: R and t must be torch tensors")
    R, batched = _device_f64(R, "R", ((3, 3),), False)
    t, t_batched = _device_f64(t, "t", ((3,), (3, 1)), False)
    T_gt, T_batched = _device_f64(T_gt, "T_gt", ((3, 4), (4, 4)), True)
    B = int(R.shape[0]) if batched else 1
    if t_batched != batched or T_batched != batched or (batched and (t.shape[0] != B or T_gt.shape[0] != B)):
        raise ValueError(f"roma_amd.metrics: R {tuple(R.shape)}, t {tuple(t.shape)} and T_gt {tuple(T_gt.shape)} do not describe the same pairs")
    _ok_shape(ok, B, batched)
    _batch_check(B, "pairs")
    t_rows = int(T_gt.shape[-2])
    # ---- nothing above touches the device
    R = _estimate(R, "R")
    dev = R.device
    R, t = _upload(R, "R", dev, (B, 3, 3)), _upload(_estimate(t, "t"), "t", dev, (B, 3))
    T_gt = _upload(T_gt, "T_gt", dev, (B, t_rows, 4))
    ok = _ok_bytes(ok, B, dev)
    log_args = _log_args(log, dev)
    err = torch.empty((B, 3), device=dev, dtype=torch.float64)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_pose_error(_ptr(R), _ptr(t), _ptr(ok), _ptr(T_gt), t_rows, B, _ptr(err), *log_args,
                                                      _stream(dev)))
        if log is not None:
            log._appended += B
    e = err.unbind(dim=1)
    return PoseError(*e) if batched else PoseError(*(x[0] for x in e))


def compute_pose_error(T_0to1, R, t):
    """romatch/utils/utils.py:126-132 with its signature: (error_t, error_R) in degrees, on the device (see `pose_error`)."""
    e = pose_error(R, t, T_0to1)
    return e.e_t, e.e_R


def homography_corner_error(H_pred, H_gt, sizes, ok=None, log=None):
    """The corner distance of the reference's HPatches benchmark (hpatches_sequences_homog_benchmark.py:89-104) on the device
    (`roma_op_corner_error`): the corners (0, 0), (0, h1 - 1), (w1 - 1, 0), (w1 - 1, h1 - 1) of image A through H_gt and through
    H_pred, the mean of the four distances divided by min(w2, h2) / 480.  H_pred [B, 3, 3] as `find_homography` returns it (a
    device tensor); H_gt [B, 3, 3] and sizes [B, 4] = (w1, h1, w2, h2), device tensors or numpy; ok bool [B]: a pair with ok
    False is scored with the reference's stand-in [[0, 0, 0], [0, 0, 0], [0, 0, 1]].  log: an `ErrorLog` to append to.

    Returns float64 [B] (0-dim for the unbatched form).  A zero third coordinate gives inf or NaN, as in the reference."""
    _log_check(log)
    if not isinstance(H_pred, torch.Tensor):
        raise TypeError(f"roma_amd.metrics: H_pred must be a torch tensor, got {type(H_pred).__name__}")
    H_pred, batched = _device_f64(H_pred, "H_pred", ((3, 3),), False)
    H_gt, g_batched = _device_f64(H_gt, "H_gt", ((3, 3),), True)
    sizes, s_batched = _device_f64(sizes, "sizes", ((4,),), True)
    B = int(H_pred.shape[0]) if batched else 1
    if g_batched != batched or s_batched != batched or (batched and (H_gt.shape[0] != B or sizes.shape[0] != B)):
        raise ValueError(f"roma_amd.metrics: H_pred {tuple(H_pred.shape)}, H_gt {tuple(H_gt.shape)} and sizes {tuple(sizes.shape)} do not "
                         "describe the same pairs")
    _ok_shape(ok, B, batched)
    _batch_check(B, "pairs")
    # ---- nothing above touches the device
    H_pred = _estimate(H_pred, "H_pred")
    dev = H_pred.device
    H_pred, H_gt, sizes = _upload(H_pred, "H_pred", dev, (B, 3, 3)), _upload(H_gt, "H_gt", dev, (B, 3, 3)), _upload(sizes, "sizes", dev, (B, 4))
    ok = _ok_bytes(ok, B, dev)
    log_args = _log_args(log, dev)
    err = torch.empty((B,), device=dev, dtype=torch.float64)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().roma_op_corner_error(_ptr(H_pred), _ptr(ok), _ptr(H_gt), _ptr(sizes), B, _ptr(err), *log_args,
                                                        _stream(dev)))
        if log is not None:
            log._appended += B
    return err if batched else err[0]


def _thresholds(thresholds):
    thr = tuple(float(x) for x in thresholds)
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError(f"roma_amd.metrics: between 1 and {MAX_THRESHOLDS} thresholds, got {len(thr)}")
    if not all(0 < x < float("inf") for x in thr):
        raise ValueError("roma_amd.metrics: thresholds must be positive and finite")
    return thr


def _summary(errors, n, state, capacity, thr, dev):
    """roma_op_error_summary: (n int64 [], below int64 [T], acc float64 [T], auc float64 [T]) on the device"""
    T = len(thr)
    out_n = torch.empty((), device=dev, dtype=torch.int64)
    below = torch.empty((T,), device=dev, dtype=torch.int64)
    acc = torch.empty((T,), device=dev, dtype=torch.float64)
    auc = torch.empty((T,), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().roma_op_error_summary(_ptr(errors), n, _ptr(state), capacity, (C.c_double * T)(*thr), T, _ptr(out_n),
                                                     _ptr(below), _ptr(acc), _ptr(auc), _stream(dev)))
    return out_n, below, acc, auc


def _errors_check(errors, name):
    if not isinstance(errors, torch.Tensor):
        raise TypeError(f"roma_amd.metrics: {name} must be a torch tensor, got {type(errors).__name__}")
    if errors.dim() != 1 or not errors.dtype.is_floating_point:
        raise ValueError(f"roma_amd.metrics: {name} must be a floating-point tensor [n], got {errors.dtype} {tuple(errors.shape)}")


def pose_auc(errors, thresholds):
    """The reference's `pose_auc` (romatch/utils/utils.py:135-147) on the device without a sort (`roma_op_error_summary`): for each
    threshold the area under the recall curve from 0 to it, over the threshold.  errors: a device tensor [n], n <= 65536, not
    negative (NaN and inf count in n and are never below a threshold); thresholds: up to 16 positive numbers.  Returns float64
    [T] on the device - the caller's `.tolist()` is the read.  n = 0 gives NaN (the reference returns 0 there)."""
    thr = _thresholds(thresholds)
    _errors_check(errors, "errors")
    n = int(errors.shape[0])
    if n > MAX_ERRORS:
        raise ValueError(f"roma_amd.metrics: {n} errors is more than one summary takes (n <= {MAX_ERRORS})")
    # ---- nothing above touches the device
    errors = _upload(errors, "errors", errors.device, (n,))
    return _summary(errors, n, None, 0, thr, errors.device)[3]


class ErrorLog:
    """The errors of a benchmark run, kept on the device: float64 rows [capacity] and the cursor {count, dropped}, which the
    appending launches read and move themselves (`pose_error(log=)`, `homography_corner_error(log=)`, `append`) - no host
    value takes part, so a loop of batches is enqueue-only.  Values past the capacity are dropped and counted.
    capacity <= 65536, what one summary takes (the largest benchmark of the reference makes 9 000 errors)."""

    def __init__(self, capacity=MAX_ERRORS, device="cuda"):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_ERRORS:
            raise ValueError(f"roma_amd.metrics: the capacity of an ErrorLog must lie in [1, {MAX_ERRORS}], got {capacity}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.RomaHipError(f"roma_amd.metrics: an ErrorLog lives on a HIP device, not on {device}; there is no CPU fallback")
        self.capacity = capacity
        self._rows = torch.zeros((capacity,), device=device, dtype=torch.float64)
        self._state = torch.zeros((2,), device=device, dtype=torch.int64)
        self.device = self._rows.device
        self._appended = 0  # values this object's calls appended: only the length of the errors() view

    def append(self, values):
        """Append float64 values [B] that are already on the device (`roma_op_error_log_append`): errors the caller computed
        some other way, or the ScanNet loop's second copy of a pair's last error.  Returns self."""
        _errors_check(values, "values")
        B = int(values.shape[0])
        _batch_check(B, "values")
        # ---- nothing above touches the device
        values = _upload(_estimate(values, "values"), "values", self.device, (B,))
        if B > 0:
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().roma_op_error_log_append(_ptr(values), B, *_log_args(self, self.device), _stream(self.device)))
            self._appended += B
        return self

    def errors(self):
        """A view of the rows appended so far through this object (at most `capacity`), in append order; no copy, no read."""
        return self._rows[:min(self._appended, self.capacity)]

    def summary(self, thresholds):
        """`roma_op_error_summary` over the rows the device cursor counts: ErrorSummary(n int64 [], dropped int64 [], below int64
        [T], acc float64 [T] = below / n, auc float64 [T] = pose_auc) on the device, one launch, no read."""
        thr = _thresholds(thresholds)
        n, below, acc, auc = _summary(self._rows, 0, self._state, self.capacity, thr, self.device)
        return ErrorSummary(n, self._state[1].clone(), below, acc, auc)

    def _read(self, thresholds):
        """the one host read of a run: (n, dropped, below, acc, auc) as Python numbers; raises if anything was dropped"""
        s = self.summary(thresholds)
        T = len(thresholds)
        flat = torch.cat((s.n.reshape(1).double(), s.dropped.reshape(1).double(), s.acc, s.auc)).tolist()
        if flat[1] > 0:
            raise _lib.RomaHipError(f"roma_amd.metrics: the ErrorLog of capacity {self.capacity} dropped {int(flat[1])} errors; "
                                    "a summary of the rest would not be the benchmark's")
        return flat[2:2 + T], flat[2 + T:]

    def pose_summary(self):
        """The dict the reference's MegaDepth and ScanNet pose benchmarks return (megadepth_pose_estimation_benchmark.py:99-116),
        as Python floats: auc_5 / auc_10 / auc_20 and map_5 = acc_5, map_10 = mean(acc_5, acc_10), map_20 = mean(acc_5, acc_10,
        acc_15, acc_20).  This is the host read of the run.  Raises if the log dropped an error."""
        acc, auc = self._read(POSE_THRESHOLDS)
        return {"auc_5": auc[0], "auc_10": auc[1], "auc_20": auc[3], "map_5": acc[0], "map_10": float(np.mean(acc[:2])),
                "map_20": float(np.mean(acc))}

    def homography_summary(self):
        """The dict the reference's HPatches benchmark returns (hpatches_sequences_homog_benchmark.py:107-113): the AUC at 3, 5 and
        10 of thresholds 1 .. 10.  This is the host read of the run.  Raises if the log dropped an error."""
        _, auc = self._read(HOMOGRAPHY_THRESHOLDS)
        return {"hpatches_homog_auc_3": auc[2], "hpatches_homog_auc_5": auc[4], "hpatches_homog_auc_10": auc[9]}


def hpatches_coordinates(matches, w1, h1, w2, h2):
    """`convert_coordinates` of the HPatches benchmark (hpatches_sequences_homog_benchmark.py:32-54), also what the ScanNet loop does
    (scannet_benchmark.py:77-97): normalised matches [..., 4] to pixels whose origin is the centre of the top-left pixel -
    `to_pixel_coordinates` minus 0.5.  Elementwise torch on the tensor's device; returns (kpts_A, kpts_B), each [..., 2]."""
    if not isinstance(matches, torch.Tensor) or matches.dim() < 1 or matches.shape[-1] != 4:
        raise ValueError("roma_amd.metrics: matches must be a tensor [..., 4]")
    offset = 0.5
    kpts_A = torch.stack((w1 * (matches[..., 0] + 1) / 2, h1 * (matches[..., 1] + 1) / 2), dim=-1) - offset
    kpts_B = torch.stack((w2 * (matches[..., 2] + 1) / 2, h2 * (matches[..., 3] + 1) / 2), dim=-1) - offset
    return kpts_A, kpts_B
