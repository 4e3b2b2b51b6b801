"""torch.multinomial(weights, k, replacement=False) on the device (`roma_op_multinomial`): the two draws of
RegressionMatcher.sample / TinyRoMa.sample (romatch/models/matcher.py:615-627, tiny.py:259-273).

Exponential race + radix select in HIP (csrc/sampling.hip), no sort and no host synchronisation.  The seed of every draw
comes from torch's CPU generator, so `torch.manual_seed(s)` makes a sampling sequence reproducible; the stream of random
numbers is not torch's, parity with the reference is distributional (as for any multinomial on another device)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def multinomial(weights: torch.Tensor, num_samples: int, generator=None) -> torch.Tensor:
    """Indices [num_samples] (int64, distinct, in draw order like torch.multinomial) drawn without replacement with probability proportional to
    `weights` [n] (>= 0).  Like torch on a GPU, the number of positive weights is not checked (no host synchronisation):
    if fewer than num_samples are positive, zero-weight entries complete the sample."""
    if not weights.is_cuda:
        raise _lib.RomaHipError("roma_amd.multinomial: weights must live on a HIP device; there is no CPU fallback")
    if weights.dim() != 1:
        raise ValueError("roma_amd.multinomial: expected a 1-D weight vector")
    n, k = int(weights.shape[0]), int(num_samples)
    if k <= 0 or k > n:
        raise RuntimeError("cannot sample n_sample > prob_dist.size(-1) samples without replacement")
    lib = _lib.load()
    w = weights.detach().to(torch.float32).contiguous()
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())  # CPU generator: no device synchronisation
    dev = w.device
    out = torch.empty((k,), device=dev, dtype=torch.int64)
    nws = int(lib.roma_op_multinomial_workspace(n, k))
    ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(lib.roma_op_multinomial(C.c_void_p(w.data_ptr()), n, k, C.c_ulonglong(seed), C.c_void_p(out.data_ptr()),
                                           C.c_void_p(ws.data_ptr()), nws, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


SAMPLE_MODES = ("threshold_balanced", "threshold", "balanced", "plain")  # the substrings decide, as in the reference
MAX_FIRST_DRAW = 65536  # csrc/sample_batched.hip SAMPLE_BATCHED_MAX_K


def sample_matches(matches: torch.Tensor, certainty: torch.Tensor, num: int = 10000, sample_mode: str = "threshold_balanced",
                   sample_thresh: float = 0.05, seed=None, return_counts: bool = False, return_indices: bool = False,
                   batched=None, _stages: bool = False):
    """RegressionMatcher.sample (romatch/models/matcher.py:598-629) applied to each pair of a batch separately, in one enqueue
    (`roma_op_sample_matches`, csrc/sample_batched.hip): no loop over pairs, no host synchronisation, and - unlike `sample()` -
    reproducible: the result of a pair is a function of its inputs and its seed alone, bit-identical from run to run, for every
    batch size and every position in the batch.  The definition is stated in include/roma_hip.h and restated in numpy by
    tools/sample_ref.py.

    matches [B, H, W, 4] with certainty [B, H, W], or [B, n, 4] with [B, n]; the single-pair forms [n, 4] and - with
    batched=False, since its rank cannot tell it from [B, n, 4] - [H, W, 4] return single-pair results.  Device tensors only. sample_mode: "threshold" in it replaces certainties above sample_thresh by 1,
    "balanced" in it draws 4 num rows first and then num of those with weight 1 / (density + 1).  seed: an int (every pair), a [B]
    tensor (one per pair) or None (drawn from torch's CPU generator), as for `roma_amd.find_homography`.

    Returns (matches [B, m, 4] float32, certainty [B, m] float32) with m = min(num, n), in draw order; with return_counts also
    counts [B] int32, the number of leading rows that are real matches (fewer than m only for a pair with fewer than m positive
    certainties; the rows behind them have zero certainty) - pass it on as `counts=`; with return_indices also idx [B, m] int64,
    the rows' indices into the pair's n rows.  The first draw is limited to 65 536 rows (num <= 16 384 in the balanced modes
    unless n is smaller): beyond that use `sample()` per pair.

        warp, certainty = model.match(im_A, im_B)                                    # [B, H, W, 4], [B, H, W]
        m, c, counts = model.sample_batched(warp, certainty, num=5000, seed=0, return_counts=True)
        kpts_A, kpts_B = model.to_pixel_coordinates(m, H_A, W_A, H_B, W_B)          # [B, 5000, 2] each
        R, t, mask, ok = roma_amd.estimate_pose(kpts_A, kpts_B, K_A, K_B, norm_thresh, counts=counts)
    """
    for t in (matches, certainty):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.RomaHipError("roma_amd.sample_matches: tensors must live on a HIP device; there is no CPU fallback")
    if matches.shape[-1] != 4 or tuple(matches.shape[:-1]) != tuple(certainty.shape) or certainty.dim() not in (1, 2, 3):
        raise ValueError(f"roma_amd.sample_matches: expected matches [..., 4] and certainty [...] of [B, H, W], [B, n], [H, W] or "
                         f"[n], got {tuple(matches.shape)} and {tuple(certainty.shape)}")
    if matches.device != certainty.device:
        raise ValueError("roma_amd.sample_matches: matches and certainty live on different devices")
    # a 3-D matches tensor is [B, n, 4] or [H, W, 4]: its rank cannot tell, so it is a batch unless batched=False says otherwise
    single = certainty.dim() == 1 if batched is None else not batched
    if (single and certainty.dim() == 3) or (not single and certainty.dim() == 1):
        raise ValueError(f"roma_amd.sample_matches: batched={batched} does not fit matches {tuple(matches.shape)}")
    B = 1 if single else int(certainty.shape[0])
    num = int(num)
    if num <= 0:
        raise ValueError("roma_amd.sample_matches: num must be positive")
    dev = matches.device
    m32 = matches.detach().to(torch.float32).reshape(B, -1, 4).contiguous()
    c32 = certainty.detach().to(torch.float32).reshape(B, -1).contiguous()
    n = int(c32.shape[1])
    balanced, threshold = "balanced" in sample_mode, "threshold" in sample_mode
    k = min(4 * num if balanced else num, n)
    m = min(num, k)
    if k > MAX_FIRST_DRAW:
        raise ValueError(f"roma_amd.sample_matches: the first draw would take {k} rows per pair; more than {MAX_FIRST_DRAW} "
                         f"(num > {MAX_FIRST_DRAW // 4} in the balanced modes) is not batched - use sample() per pair")
    out_m = torch.empty((B, m, 4), device=dev, dtype=torch.float32)
    out_c = torch.empty((B, m), device=dev, dtype=torch.float32)
    counts = torch.zeros((B,), device=dev, dtype=torch.int32) if return_counts else None
    idx = torch.empty((B, m), device=dev, dtype=torch.int64) if return_indices else None
    # the two intermediate outputs of the C entry point, for the tests of the stages (tests/test_gpu_sample_batched.py)
    first_idx = torch.empty((B, k), device=dev, dtype=torch.int64) if _stages else None
    density = torch.zeros((B, k), device=dev, dtype=torch.float32) if _stages else None
    if B > 0 and n > 0:
        from .geometry import _seeds
        seeds = _seeds(seed, B, dev)
        lib = _lib.load()
        nws = int(lib.roma_op_sample_matches_workspace(B, n, num, int(balanced)))
        ws = torch.empty((nws,), device=dev, dtype=torch.uint8)
        P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(lib.roma_op_sample_matches(P(m32), P(c32), P(seeds), B, n, num, int(threshold), float(sample_thresh),
                                                  int(balanced), P(out_m), P(out_c), P(counts), P(idx), P(first_idx), P(density),
                                                  P(ws), nws, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    out = (out_m, out_c) + ((counts,) if return_counts else ()) + ((idx,) if return_indices else ())
    out = out + ((first_idx, density) if _stages else ())
    return tuple(o[0] for o in out) if single else out
