"""Image preprocessing on the device (`roma_op_preprocess`, csrc/preprocess.hip): the PIL bicubic resize, the / 255 and the ImageNet
normalisation that `RegressionMatcher.match()` does on the host for one image at a time (`matcher._pil_to_normalised`), for a whole
batch of decoded images of mixed sizes and for up to two target sizes from one upload - bit-identical to the host path.

Pillow resizes 8-bit images in fixed point, horizontally first, then vertically, and rounds to uint8 between the two passes; the
kernels do exactly that (the definition is in include/roma_hip.h, restated in numpy by tools/pil_resample_ref.py).  Decoding
(JPEG / PNG) stays on the host, where callers can thread it."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib

DESC_BYTES = 24  # one descriptor: int64 {byte offset, H, W}


def _as_sizes(sizes):
    """((h, w),) or ((h, w), (h, w)), and whether a single size was given"""
    try:
        single = len(sizes) == 2 and all(isinstance(v, (int, np.integer)) for v in sizes)
        out = (tuple(sizes),) if single else tuple(tuple(s) for s in sizes)
        ok = len(out) in (1, 2) and all(len(s) == 2 and all(isinstance(v, (int, np.integer)) and v >= 1 for v in s) for s in out)
    except TypeError:
        ok, single, out = False, False, ()
    if not ok:
        raise ValueError(f"preprocess_images: sizes must be (h, w) or a pair of them with positive integers, got {sizes!r}")
    return tuple((int(h), int(w)) for h, w in out), single


def _as_uint8_hwc(im, i):
    """uint8 [H, W, 3]: a contiguous numpy array for a host image, the tensor itself for a device tensor"""
    from PIL import Image
    from .matcher import _check_input
    if isinstance(im, (str, os.PathLike, Image.Image)):
        return np.ascontiguousarray(np.asarray(_check_input(im), dtype=np.uint8))  # NotImplementedError: 16-bit / non-RGB
    if isinstance(im, torch.Tensor):
        shape, dtype, good = tuple(im.shape), im.dtype, torch.uint8
    elif isinstance(im, np.ndarray):
        shape, dtype, good = im.shape, im.dtype, np.uint8
    else:
        raise ValueError(f"preprocess_images: image {i} is a {type(im).__name__}; expected a path, a PIL image, a uint8 ndarray "
                         "[H, W, 3] or a uint8 tensor [H, W, 3]")
    if dtype != good:
        raise ValueError(f"preprocess_images: image {i} has dtype {dtype}, expected uint8")
    if len(shape) != 3:
        raise ValueError(f"preprocess_images: image {i} has rank {len(shape)}, expected [H, W, 3]")
    if shape[2] != 3:
        raise ValueError(f"preprocess_images: image {i} has {shape[2]} channels, expected 3 (shape [H, W, 3])")
    if shape[0] < 1 or shape[1] < 1 or shape[0] > 32768 or shape[1] > 32768:
        raise ValueError(f"preprocess_images: image {i} is {shape[0]} x {shape[1]}; sides must lie in [1, 32768]")
    if isinstance(im, torch.Tensor):
        return im.detach() if im.is_cuda else np.ascontiguousarray(im.detach().numpy())
    return np.ascontiguousarray(im)


def preprocess_images(images, sizes, *, normalize=True, device=None):
    """Resize and normalise a batch of decoded RGB images on the device, exactly as the host path of `match()` does.

    images: a sequence of paths, PIL RGB images, uint8 ndarrays [H, W, 3] or uint8 tensors [H, W, 3] (host or device); the sizes may
    differ from image to image.  sizes: (h, w), or a pair of them (e.g. the coarse and the upsample resolution of a matcher: both
    come from the same upload).  normalize=False stops after the / 255 (what `visualize_warp` takes).

    Returns a float32 device tensor [N, 3, h, w] for one size, a tuple of two for a pair - every bit equal to
    `_pil_to_normalised(image, (h, w))`.  Host images are packed, with the descriptor table, into one pinned buffer and uploaded
    once; device tensors are packed on the device.  One enqueue of three kernels on the current stream, no host synchronisation.

    Raises NotImplementedError for 16-bit and non-RGB PIL images (as `match()` does), ValueError - before any device work - for a
    wrong dtype, rank or channel count, an empty list or bad sizes."""
    sizes, single = _as_sizes(sizes)
    if isinstance(images, (str, os.PathLike, np.ndarray, torch.Tensor)) or not hasattr(images, "__len__"):
        raise ValueError("preprocess_images: images must be a sequence of images")
    if len(images) == 0:
        raise ValueError("preprocess_images: the list of images is empty")
    if len(images) > 65535:
        raise ValueError("preprocess_images: at most 65535 images per call")
    ims = [_as_uint8_hwc(im, i) for i, im in enumerate(images)]
    on_dev = [im for im in ims if isinstance(im, torch.Tensor)]
    if device is None:
        device = on_dev[0].device if on_dev else "cuda"
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.RomaHipError(f"roma_amd.preprocess_images runs only on a HIP device (got device={device!r}); there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    for im in on_dev:
        if im.device != dev:
            raise ValueError(f"preprocess_images: a tensor lives on {im.device}, the call runs on {dev}")

    # one buffer: [descriptor table][host images][device images]; offsets are relative to the buffer, images are packed tightly
    n = len(ims)
    desc = np.zeros((n, 3), dtype=np.int64)
    at = DESC_BYTES * n
    for host_pass in (True, False):
        for i, im in enumerate(ims):
            if isinstance(im, np.ndarray) == host_pass:
                desc[i] = (at, im.shape[0], im.shape[1])
                at += 3 * im.shape[0] * im.shape[1]
        if host_pass:
            host_bytes = at
    total = at
    lib = _lib.load()
    targets = (C.c_int * (2 * len(sizes)))(*[v for s in sizes for v in s])
    desc_p = desc.ctypes.data_as(C.c_void_p)
    ws_bytes = lib.roma_op_preprocess_workspace(desc_p, n, targets, len(sizes))
    if ws_bytes < 0:
        raise ValueError(_lib.last_error(lib))
    with torch.cuda.device(dev):
        staging = torch.empty(host_bytes, dtype=torch.uint8, pin_memory=True)
        flat = staging.numpy()
        flat[:DESC_BYTES * n] = desc.reshape(-1).view(np.uint8)
        for i, im in enumerate(ims):
            if isinstance(im, np.ndarray):
                flat[desc[i, 0]:desc[i, 0] + im.size] = im.reshape(-1)
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        buf[:host_bytes].copy_(staging, non_blocking=True)  # the one upload
        for i, im in enumerate(ims):
            if isinstance(im, torch.Tensor):
                buf[desc[i, 0]:desc[i, 0] + im.numel()].copy_(im.reshape(-1))
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=dev)
        outs = [torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) for h, w in sizes]
        _lib.check(lib.roma_op_preprocess(C.c_void_p(buf.data_ptr()), total, desc_p, C.c_void_p(buf.data_ptr()), n, targets, len(sizes),
                                          int(bool(normalize)), C.c_void_p(outs[0].data_ptr()),
                                          C.c_void_p(outs[1].data_ptr()) if len(outs) == 2 else None, C.c_void_p(ws.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), lib=lib)
    return outs[0] if single else tuple(outs)
