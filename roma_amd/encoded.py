"""Cached per-image features for image sets: `RegressionMatcher.encode_images` runs the encoders and the proj heads once per
image, `match_pairs` matches any pairs of the encoded images (include/roma_hip.h: roma_encode / roma_match_encoded).

This module is the host side of it: the pair list, the layout of one image's feature pack (a pure Python restatement of
csrc/encoded.hip::pack_layout, so both can be tested without a GPU) and the `EncodedImages` record.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np

SCALES = (16, 8, 4, 2, 1)
PROJ_COUT = (512, 512, 256, 64, 9)  # csrc/arch.h: channels of the projected map of each scale
SEGMENT_ALIGN = 256


def _round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def all_pairs(n: int):
    """All (i, j) with 0 <= i < j < n in lexicographic order: n (n - 1) / 2 tuples."""
    n = int(n)
    if n < 0:
        raise ValueError(f"all_pairs: n must be >= 0 (got {n})")
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def pack_layout(coarse_hw, upsample_hw, itemsize: int):
    """Layout of one image's feature pack.  coarse_hw: (h, w) of the coarse pass; upsample_hw: (h, w) of the upsample pass, or
    None / (0, 0) for a handle without one; itemsize: bytes of an activation element (2 in the 16-bit modes, 4 in f32).

    Returns {"segments": [{"pass": 0 | 1, "scale": s, "hw": h_s * w_s, "ldf": row stride in elements, "offset": bytes,
    "bytes": hw * ldf * itemsize}, ...], "coarse_bytes": end of the coarse part, "total": bytes of the pack}.  Segments come in
    the order coarse 16, 8, 4, 2, 1, then upsample 8, 4, 2, 1; each starts on a 256-byte boundary and so does the next pack."""
    if itemsize not in (2, 4):
        raise ValueError(f"pack_layout: itemsize must be 2 or 4 (got {itemsize})")
    up = tuple(int(v) for v in upsample_hw) if upsample_hw is not None else (0, 0)
    passes = [tuple(int(v) for v in coarse_hw)] + ([up] if up[0] > 0 and up[1] > 0 else [])
    segments, off, coarse_bytes = [], 0, 0
    for ps, (H, W) in enumerate(passes):
        for si, s in enumerate(SCALES):
            if ps == 1 and s == 16:
                continue  # the upsample pass has no stride-16 scale
            hw = (H // 14) * (W // 14) if s == 16 else (H // s) * (W // s)
            ldf = _round_up(PROJ_COUT[si], 8)
            nbytes = hw * ldf * itemsize
            segments.append({"pass": ps, "scale": s, "hw": hw, "ldf": ldf, "offset": off, "bytes": nbytes})
            off = _round_up(off + nbytes, SEGMENT_ALIGN)
        if ps == 0:
            coarse_bytes = off
    return {"segments": segments, "coarse_bytes": coarse_bytes, "total": off}


def check_pairs(pairs, n: int) -> np.ndarray:
    """The pair list as a contiguous int32 array [P, 2], validated on the host: integer values, shape [P, 2] with P >= 1, every
    index in [0, n).  pairs=None: all_pairs(n).  Raises ValueError."""
    n = int(n)
    if pairs is None:
        pairs = all_pairs(n)
    if hasattr(pairs, "detach"):  # a torch tensor: host data is expected, a device tensor would need a sync to check
        if getattr(pairs, "is_cuda", False):
            raise ValueError("match_pairs: pairs is host data (a sequence or an int array [P, 2]): it is checked before anything is launched")
        pairs = pairs.detach().numpy()
    a = np.asarray(pairs)
    if a.size == 0:
        raise ValueError("match_pairs: empty pair list")
    if a.dtype.kind not in "iu":
        raise ValueError(f"match_pairs: pairs must hold integers (got dtype {a.dtype})")
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"match_pairs: pairs must have shape [P, 2] (got {tuple(a.shape)})")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= n:
        bad = a[((a < 0) | (a >= n)).any(axis=1)][0]
        raise ValueError(f"match_pairs: pair ({int(bad[0])}, {int(bad[1])}) names an image outside [0, {n})")
    return np.ascontiguousarray(a.astype(np.int32))


@dataclass
class EncodedImages:
    """What `encode_images` returns: N feature packs in one device buffer, and the handle configuration they were made for."""
    feats: Any                    # torch.uint8 tensor [N * pack_bytes] on the device (views into a caller's buffer are fine)
    n: int                        # number of images
    pack_bytes: int               # roma_encoded_bytes of the handle
    key: Tuple                    # RegressionMatcher._config_key of the handle that wrote the packs (resolutions, precision, max_batch, device)
    has_upsample: bool            # the upsample part of the packs is filled (high-resolution images were given)
    weights_id: Tuple[int, int]   # id() of the matcher / DINOv2 state dicts
    weights: Optional[Tuple] = None  # keeps those dicts alive, so that the ids stay theirs

    def __len__(self) -> int:
        return self.n
