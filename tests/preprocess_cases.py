"""The cases shared by tests/test_cpu_preprocess.py and tests/test_gpu_preprocess.py: (name, source uint8 [H, W, 3], target (h, w)).
The smallest shapes at which each part of the bicubic resize can go wrong; sources are tests/golden/pair_A.png (480 x 640), crops
of it, or default_rng(0) bytes."""
import functools
import os

import numpy as np

from conftest import GOLDEN

CLAMP_CASES = ("binary_64x80", "binary_20x24")


@functools.lru_cache(maxsize=None)
def cases():
    from PIL import Image
    pair_a = np.array(Image.open(os.path.join(GOLDEN, "pair_A.png")).convert("RGB"))
    assert pair_a.shape == (480, 640, 3)
    rng = np.random.default_rng(0)

    def crop(h, w, y0=101, x0=203):
        return np.ascontiguousarray(pair_a[y0:y0 + h, x0:x0 + w])

    every_byte = np.stack([np.roll(np.arange(256, dtype=np.uint8), 37 * c) for c in range(3)], axis=-1).reshape(16, 16, 3)
    out = [
        ("down_both", pair_a, (56, 70)),                                        # non-integer downscale on both axes
        ("up_odd", crop(37, 53), (70, 84)),                                     # upscale; rows of 159 bytes, unaligned offsets
        ("skip_vertical", pair_a, (480, 98)),                                   # one pass skipped, each way
        ("skip_horizontal", pair_a, (42, 640)),
        ("mixed", pair_a, (560, 560)),                                          # down in x, up in y
        ("copy", crop(28, 42), (28, 42)),                                       # both passes skipped
        ("tiny_5x3", crop(5, 3), (28, 42)),                                     # every window clipped at both ends
        ("width_1", crop(301, 1), (14, 14)),
        ("taps_99", rng.integers(0, 256, (97, 1031, 3), dtype=np.uint8), (28, 42)),  # 99 horizontal taps
        ("binary_64x80", (rng.integers(0, 2, (64, 80, 3)) * 255).astype(np.uint8), (42, 56)),  # overshoot: both clamps fire
        ("binary_20x24", (rng.integers(0, 2, (20, 24, 3)) * 255).astype(np.uint8), (56, 70)),
        ("every_byte", every_byte, (16, 16)),                                   # the whole normalisation table
    ]
    for _, a, _ in out:
        a.setflags(write=False)
    return tuple(out)


def reference(img, hw, normalize=True):
    """what the host path makes of the image: `_pil_to_normalised`, or resize and / 255 only - float32 [3, h, w] numpy"""
    from PIL import Image
    from roma_amd.matcher import _pil_to_normalised
    im = Image.fromarray(np.asarray(img))
    if normalize:
        return _pil_to_normalised(im, hw).numpy()
    r = im.resize((hw[1], hw[0]), resample=Image.BICUBIC)
    return np.array(r, dtype=np.float32).transpose((2, 0, 1)) / np.float32(255.0)
