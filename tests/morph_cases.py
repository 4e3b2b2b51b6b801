"""The scene shared by tests/test_cpu_morph.py and tests/test_gpu_morph.py (and recorded, with the frames torch's grid_sample and the
reference's tensor_to_pil make of it, in tests/golden/morph_reference.npz by tools/make_morph_goldens.py).  The smallest scene that
takes every branch of roma_op_render_morph:

  warp       B = 2 pairs of 37 x 53: W is odd, 37 * 53 = 1961 = 7 waves of 256 pixels + 169 pixels in two workgroups, so the last
             wave of a frame is partial, and 1961 * 3 bytes per frame is odd, so frames start at every dword phase: the dword and the
             byte store path both run, for full and for partial waves.  Columns 0:2 are the pixel-centre grid; columns 2:4 are
             (1.15 x + 0.12 sin 3y + 0.05, 1.1 y - 0.1 cos 2x - 0.08) (pair 1: the signs of the three small terms flipped), which
             reaches about 1.3: pixels with all four taps outside, with one to three outside, and inside;
  image      29 x 41 (another size and aspect than the warp), uniform random float32 - a picture derived from uint8 would put many
             values of 255 v exactly on integers; `image_u8` is a second, uint8 picture for the uint8-input form;
  ts         morph_times(7) (t = 1, t = 0 and values with rounding in 1 - t) plus 1.5 and -0.25: T = 9;
  certainty  smooth in [0, 1] with exact zeros and ones, background 1, on three of the times (TS_CERT);
  ts_one     T = 1;  ts_chunk  T = FRAME_CHUNK + 1, which needs a second frame chunk."""
import functools
import os
import sys

import numpy as np

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import morph_ref as mr  # noqa: E402

B, H, W = 2, 37, 53
IM_H, IM_W = 29, 41
BACKGROUND = 1.0
GOLDEN_FILE = os.path.join(GOLDEN, "morph_reference.npz")
INPUTS = ("warp", "image", "image_u8", "ts", "certainty", "ts_cert")
FLOAT_ATOL = 2e-6        # float frames: the bound the project holds visualize_warp to
U8_MARGIN = 1e-3         # uint8 frames: 255 v this close to an integer may fall to either level (255 * 2e-6 = 5.1e-4)
U8_EXCUSED_SHARE = 0.005


def build_scene():
    """the scene from its seeds - what tools/make_morph_goldens.py records"""
    rng = np.random.default_rng(2024)
    xs = ((2.0 * np.arange(W) + 1.0) / W - 1.0).astype(np.float32)
    ys = ((2.0 * np.arange(H) + 1.0) / H - 1.0).astype(np.float32)
    y, x = np.meshgrid(ys.astype(np.float64), xs.astype(np.float64), indexing="ij")
    warp = np.empty((B, H, W, 4), dtype=np.float32)
    for b, s in enumerate((1.0, -1.0)):
        warp[b, ..., 0], warp[b, ..., 1] = x, y
        warp[b, ..., 2] = 1.15 * x + s * 0.12 * np.sin(3 * y) + s * 0.05
        warp[b, ..., 3] = 1.1 * y - s * 0.1 * np.cos(2 * x) - s * 0.08
    image = rng.random((B, 3, IM_H, IM_W), dtype=np.float32)
    image_u8 = rng.integers(0, 256, (B, IM_H, IM_W, 3), dtype=np.uint8)
    ts = np.concatenate([mr.morph_times(7), [1.5, -0.25]])
    cert = np.clip(0.5 + 0.7 * np.sin(2.5 * x + 0.3)[None] * np.cos(3.0 * y - 0.2)[None] * np.array([1.0, -1.0])[:, None, None], 0.0, 1.0)
    return {"warp": warp, "image": image, "image_u8": image_u8, "ts": ts, "certainty": cert.astype(np.float32),
            "ts_cert": ts[[1, 4, 7]].copy()}


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/morph_reference.npz: the scene (in_*) and the reference's frames on it (ref_*), read-only"""
    with np.load(GOLDEN_FILE) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene():
    """the recorded scene (the bits the reference ran on, whatever this machine's libm makes of build_scene)"""
    g = golden()
    return {k: g["in_" + k] for k in INPUTS}


def extra_times(chunk):
    """(ts_one [1], ts_chunk [chunk + 1]): a single frame, and one frame more than a workgroup's chunk"""
    return np.array([0.3]), np.linspace(-0.1, 1.1, chunk + 1)


def _render(s, image, ts, certainty=None):
    f, u = zip(*(mr.render_morph(s["warp"][b], image[b], ts, None if certainty is None else certainty[b], BACKGROUND) for b in range(B)))
    out = (np.stack(f), np.stack(u))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, chunk=None):
    """what tools/morph_ref.py makes of the scene, computed once per form: (float frames [B, T, 3, H, W], uint8 frames [B, T, H, W, 3])
    for name in plain, cert, u8 (the uint8 picture), one, chunk (the last two need the frame chunk)"""
    s = scene()
    if name == "plain":
        return _render(s, s["image"], s["ts"])
    if name == "cert":
        return _render(s, s["image"], s["ts_cert"], s["certainty"])
    if name == "u8":
        return _render(s, s["image_u8"], s["ts"])
    one, many = extra_times(chunk)
    return _render(s, s["image"], one if name == "one" else many)


def check_uint8(got, ref_u8, ref_float, what=""):
    """the uint8 comparison rule.  got, ref_u8 uint8 [..., H, W, 3]; ref_float the recorded float frames [..., 3, H, W].  Returns the
    share of excused values (those that may differ by one level) and the number that do differ."""
    ref_float = np.moveaxis(ref_float, -3, -1)
    assert got.shape == ref_u8.shape == ref_float.shape and got.dtype == np.uint8, what
    exc = mr.excused(ref_float, U8_MARGIN)
    d = np.abs(got.astype(np.int16) - ref_u8.astype(np.int16))
    share, n_diff = float(exc.mean()), int((d != 0).sum())
    print(f"{what}: uint8 frames: {n_diff} of {d.size} values differ (all by <= {int(d.max())}), {share * 100:.3f} % excused")
    assert d.max() <= 1, what
    assert not (d[~exc] != 0).any(), what  # equal wherever 255 v is not within the margin of an integer, and at exact 0 and 1
    assert share <= U8_EXCUSED_SHARE, what
    return share, n_diff
