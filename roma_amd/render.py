"""Warp morph rendering on the device (`roma_op_render_morph`, csrc/morph.hip): the frames of the reference's demo/demo_3D_effect.py -
`F.grid_sample(image, (1 - t) * warp[..., :2] + t * warp[..., 2:])` for every t of a schedule, through `tensor_to_pil` - in one
enqueue instead of several framework launches and a device-to-host copy per frame.  The warp is read once per pixel and chunk of
`FRAME_CHUNK` frames, the picture is gathered from cache, each frame byte is stored once.  The definition is stated in
include/roma_hip.h and restated in numpy float32 by tools/morph_ref.py.

Conventions are those of `roma_amd.gt_warp`: device tensors only (the schedule may also be host values), nothing synchronises with
the host, and every output is bit-identical from run to run and independent of the batch a pair sits in."""
from __future__ import annotations

import math
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream

FRAME_CHUNK = 32  # frames one workgroup renders from the warp rows it loaded (roma_op_render_morph_frame_chunk)


def morph_times(n=200):
    """The schedule of the reference's demo: `(1 + cos(x)) / 2` over `linspace(0, 2 pi, n)`, float64 [n] (1 -> 0 -> 1)."""
    n = int(n)
    if n < 1:
        raise ValueError(f"roma_amd.render: morph_times needs n >= 1, got {n}")
    return (1 + np.cos(np.linspace(0, 2 * np.pi, n))) / 2


_device_tensor = partial(_lib._device_tensor, module="render")


def _times(ts):
    """the schedule as (T, device tensor or None, host float64 array or None) after its shape check"""
    if isinstance(ts, torch.Tensor) and ts.is_cuda:
        if ts.dim() != 1 or not ts.dtype.is_floating_point:
            raise ValueError(f"roma_amd.render: ts must be a floating-point [T] tensor, got {ts.dtype} {tuple(ts.shape)}")
        return int(ts.shape[0]), ts, None
    host = np.array(ts.detach().numpy() if isinstance(ts, torch.Tensor) else ts, dtype=np.float64, order="C")  # a copy
    if host.ndim != 1:
        raise ValueError(f"roma_amd.render: ts must be a sequence of T times, got shape {host.shape}")
    return int(host.shape[0]), None, host


def render_morph(warp, image, ts, *, certainty=None, background=1.0, dtype=torch.uint8):
    """The frames `grid_sample(image, (1 - t) * warp[..., :2] + t * warp[..., 2:])` for every t in ts (bilinear, align_corners=False,
    zeros padding), in one enqueue (`roma_op_render_morph`).

    warp       float32 [B, H, W, 4] or [H, W, 4] as `match()` returns it, read in place - also the left half `warp[:, :, :W]` of a
               symmetric warp (any row and batch stride);
    image      the picture that columns 2:4 point into (image B): float32 [B, 3, h, w] in [0, 1], or uint8 [B, h, w, 3] as decoded
               (used as float(u) / 255, the same bits as the float32 form of the same picture); (h, w) need not be (H, W); without a
               batch axis where warp has none;
    ts         T times - a host sequence, a numpy array or a device tensor; any real value (0 shows columns 0:2, 1 columns 2:4);
    certainty  optional float32 [B, H, W] (or [H, W]): frames are blended as certainty * frame + (1 - certainty) * background,
               as `visualize_warp` blends over white;
    dtype      torch.uint8 (default): [B, T, H, W, 3], min(max(v, 0), 1) * 255 truncated - what the reference's `tensor_to_pil`
               makes of a frame, ready for Pillow or an encoder; torch.float32: [B, T, 3, H, W], the frames before that step.

    The batch axis is dropped when warp has none.  T is split into chunks of `FRAME_CHUNK` frames across workgroups."""
    if not isinstance(warp, torch.Tensor) or not isinstance(image, torch.Tensor):
        raise TypeError("roma_amd.render: warp and image must be torch tensors")
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"roma_amd.render: dtype must be torch.uint8 or torch.float32, got {dtype}")
    background = float(background)
    if math.isnan(background):
        raise ValueError("roma_amd.render: background is NaN")
    batched = warp.dim() == 4
    if warp.dim() not in (3, 4) or warp.shape[-1] != 4 or warp.dtype != torch.float32 or min(warp.shape) < 1:
        raise ValueError(f"roma_amd.render: warp must be float32 [B, H, W, 4] or [H, W, 4], got {warp.dtype} {tuple(warp.shape)}")
    if not batched:
        warp = warp[None]
    B, H, W = (int(x) for x in warp.shape[:3])
    if image.dtype not in (torch.float32, torch.uint8) or image.dim() != (4 if batched else 3):
        raise ValueError("roma_amd.render: image must be float32 [B, 3, h, w] or uint8 [B, h, w, 3] (without B where warp has none), got "
                         f"{image.dtype} {tuple(image.shape)}")
    if not batched:
        image = image[None]
    image_u8 = image.dtype == torch.uint8
    if int(image.shape[0]) != B or int(image.shape[3 if image_u8 else 1]) != 3 or min(image.shape) < 1:
        raise ValueError(f"roma_amd.render: image must be float32 [{B}, 3, h, w] or uint8 [{B}, h, w, 3], got {image.dtype} {tuple(image.shape)}")
    h, w = (int(x) for x in (image.shape[1:3] if image_u8 else image.shape[2:4]))
    if certainty is not None:
        if not isinstance(certainty, torch.Tensor):
            raise TypeError(f"roma_amd.render: certainty must be a torch tensor, got {type(certainty).__name__}")
        if not batched and certainty.dim() == 2:
            certainty = certainty[None]
        if certainty.dtype != torch.float32 or tuple(certainty.shape) != (B, H, W):
            raise ValueError(f"roma_amd.render: certainty must be float32 {[B, H, W]}, got {certainty.dtype} {tuple(certainty.shape)}")
    T, ts_dev, ts_host = _times(ts)
    if T < 1:
        raise ValueError("roma_amd.render: ts must hold at least one time")
    if B > 65535 or max(H, W, h, w) > 32768 or T > 65535 * FRAME_CHUNK:
        raise ValueError(f"roma_amd.render: B = {B}, T = {T}, warp {H} x {W}, image {h} x {w} is more than one call takes "
                         f"(B <= 65535, T <= {65535 * FRAME_CHUNK}, sides <= 32768)")
    # ---- nothing above touches the device
    warp = _device_tensor(warp, "warp")
    dev = warp.device
    image = _device_tensor(image, "image").contiguous()
    sb, sr, sc, se = warp.stride()
    sc, sr = (4 if W == 1 else sc), (4 * W if H == 1 else sr)  # the stride of an axis of length 1 is never used
    sb = H * sr if B == 1 else sb
    in_place = se == 1 and sc == 4 and sr % 4 == 0 and sb % 4 == 0 and sr >= 4 * W and sb >= (H - 1) * sr + 4 * W and warp.data_ptr() % 16 == 0
    if not in_place:
        warp = warp.contiguous()
        warp = warp.clone() if warp.data_ptr() % 16 else warp  # a contiguous view at an odd offset: a fresh allocation is aligned
        sb, sr = 4 * H * W, 4 * W
    cb = cr = 0
    if certainty is not None:
        certainty = _device_tensor(certainty, "certainty")
        cb, cr, cc = certainty.stride()
        cr = W if H == 1 else cr
        cb = H * cr if B == 1 else cb
        if not ((cc == 1 or W == 1) and cr >= W and cb >= (H - 1) * cr + W):
            certainty = certainty.contiguous()
            cb, cr = H * W, W
    if ts_dev is not None:
        ts_dev = ts_dev.detach().to(device=dev, dtype=torch.float64).contiguous()
    else:
        ts_dev = torch.from_numpy(ts_host).to(dev)  # one small upload, no synchronisation
    lib = _lib.load()
    ws_bytes = int(lib.roma_op_render_morph_workspace(B, h, w, T))
    if ws_bytes < 0:
        raise _lib.RomaHipError("roma_amd.render: roma_op_render_morph_workspace refused the sizes")
    ws = torch.empty((ws_bytes + 15) // 16 * 2, device=dev, dtype=torch.float64)
    out = torch.empty((B, T, H, W, 3) if dtype == torch.uint8 else (B, T, 3, H, W), device=dev, dtype=dtype)
    with torch.cuda.device(dev):
        _lib.check(lib.roma_op_render_morph(
            _ptr(warp), int(sb), int(sr), _ptr(image), int(image_u8), _ptr(ts_dev), _ptr(certainty), int(cb), int(cr), background, B, T,
            H, W, h, w, _ptr(out), int(dtype == torch.float32), _ptr(ws), ws_bytes, _stream(dev)))
    return out if batched else out[0]
