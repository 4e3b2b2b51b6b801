"""numpy float32 restatement of roma_op_render_morph (csrc/morph.hip; the definition is in include/roma_hip.h) - the oracle of
tests/test_gpu_morph.py, itself checked against recorded frames of torch's grid_sample and the reference's tensor_to_pil by
tests/test_cpu_morph.py.  Every expression is an elementwise float32 + - * floor min max in the order the kernel uses, one rounding
per operation and no fused multiply-add, so both sides round alike."""
from __future__ import annotations

import numpy as np

F = np.float32


def morph_times(n=200):
    """the schedule of the reference's demo_3D_effect.py: (1 + cos x) / 2 over linspace(0, 2 pi, n), float64"""
    return (1 + np.cos(np.linspace(0, 2 * np.pi, int(n)))) / 2


def frame_weights(ts):
    """(w0, w1) float32 [T]: 1 - t and t formed in float64 and rounded once - what the Python scalars of (1 - t) * A + t * B become
    when they multiply float32 tensors"""
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    return (1.0 - ts).astype(F), ts.astype(F)


def image_f32(image):
    """the picture as float32 [3, h, w]: a float32 planar image as it is, a uint8 [h, w, 3] image as float(u) / 255.f"""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return np.ascontiguousarray((image.astype(F) / F(255.0)).transpose(2, 0, 1))
    assert image.dtype == F and image.ndim == 3 and image.shape[0] == 3
    return image


def _unnormalise(g, size):
    i = ((g + F(1.0)) * F(size) - F(1.0)) * F(0.5)
    return np.fmin(np.fmax(i, F(-1.0e6)), F(1.0e6))  # fmax / fmin: a NaN coordinate becomes -1e6, every tap outside


def sample(image, gx, gy):
    """bilinear, align_corners=False, zeros padding, of image f32 [3, h, w] at normalised float32 gx, gy [...]: f32 [3, ...]"""
    _, h, w = image.shape
    ix, iy = _unnormalise(gx, w), _unnormalise(gy, h)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    tx, ty = ix - fx0, iy - fy0
    ux, uy = F(1.0) - tx, F(1.0) - ty
    rgb = np.zeros((3,) + gx.shape, dtype=F)
    for wgt, yy, xx in ((ux * uy, y0, x0), (tx * uy, y0, x0 + 1), (ux * ty, y0 + 1, x0), (tx * ty, y0 + 1, x0 + 1)):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = np.where(inside, image[:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], F(0.0))  # a tap outside reads 0
        rgb = rgb + wgt * v
    assert rgb.dtype == F
    return rgb


def to_uint8(v):
    """(unsigned char)(min(max(v, 0), 1) * 255): truncation, as numpy_to_pil does it after tensor_to_pil's clip; NaN -> 0"""
    return (np.fmin(np.fmax(v, F(0.0)), F(1.0)) * F(255.0)).astype(np.uint8)


def render_morph(warp, image, ts, certainty=None, background=1.0):
    """one pair: warp f32 [H, W, 4], image f32 [3, h, w] or uint8 [h, w, 3], ts [T], certainty f32 [H, W] or None.
    Returns (frames f32 [T, 3, H, W], frames uint8 [T, H, W, 3])."""
    warp = np.asarray(warp)
    assert warp.dtype == F and warp.ndim == 3 and warp.shape[-1] == 4
    img = image_f32(image)
    w0, w1 = frame_weights(ts)
    ax, ay, bx, by = (warp[..., k] for k in range(4))
    out = np.empty((len(w0), 3) + warp.shape[:2], dtype=F)
    with np.errstate(all="ignore"):
        if certainty is not None:
            ce = np.asarray(certainty)
            assert ce.dtype == F and ce.shape == warp.shape[:2]
            bg = (F(1.0) - ce) * F(background)
        for k in range(len(w0)):
            gx, gy = w0[k] * ax + w1[k] * bx, w0[k] * ay + w1[k] * by
            v = sample(img, gx, gy)
            if certainty is not None:
                v = ce * v + bg
            out[k] = v
        return out, to_uint8(out).transpose(0, 2, 3, 1).copy()


def excused(ref_float, margin=1e-3):
    """where the uint8 comparison rule allows a difference of one level: 255 v within `margin` of an integer, and v not exactly 0 or 1.
    ref_float: the recorded float frames in the layout of the uint8 frames compared"""
    v = ref_float.astype(np.float64) * 255.0
    return (np.abs(v - np.round(v)) < margin) & (ref_float != 0.0) & (ref_float != 1.0)
