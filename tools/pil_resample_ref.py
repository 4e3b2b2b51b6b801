"""Numpy restatement of Pillow's 8-bit bicubic resize of an RGB image (`Image.resize((w, h), Image.BICUBIC)`) and of the
normalisation that follows it in `roma_amd.matcher._pil_to_normalised` - the definition of `roma_op_preprocess`
(include/roma_hip.h, csrc/preprocess.hip) and the oracle of tests/test_cpu_preprocess.py.

Pillow resamples in fixed point with 22 fractional bits, in two passes: HORIZONTAL first, then VERTICAL, and the intermediate
image is rounded and clamped to uint8 between them.  An axis whose size does not change is skipped.  The coefficients of an axis
are computed in float64, every sum in index order; `(int)` truncates toward zero.

    bicubic(x), a = -0.5:  x = |x|;  x < 1: ((a+2) x - (a+3)) x x + 1;   x < 2: (((x-5) x + 8) x - 4) a;   else 0
    scale = in / out;  fs = max(scale, 1);  support = 2 fs;  ss = 1 / fs
    for each output xx:  center = (xx + 0.5) scale
        xmin = max(0, (int)(center - support + 0.5));  xmax = min(in, (int)(center + support + 0.5));  n = xmax - xmin
        k[i] = bicubic((i + xmin - center + 0.5) ss), i < n;   ww = sum k[i];   if ww != 0: k[i] /= ww
        K[i] = (int)(k[i] 2^22 + 0.5) if k[i] >= 0 else (int)(k[i] 2^22 - 0.5)
    one pass, per channel:  s = 2^21 + sum_i pixel[xmin + i] K[i]  (int32);   out = clamp(s >> 22, 0, 255)
"""
import numpy as np

PRECISION_BITS = 22
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def coefficients(n_in, n_out):
    """(xmin [n_out], n [n_out], K [n_out, max n] int32, zero beyond n) of one axis"""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    rows, xmins, ns = [], [], []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        n = xmax - xmin
        k = [bicubic((i + xmin - center + 0.5) * ss) for i in range(n)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        K = [int(v * float(1 << PRECISION_BITS) + 0.5) if v >= 0.0 else int(v * float(1 << PRECISION_BITS) - 0.5) for v in k]
        rows.append(K), xmins.append(xmin), ns.append(n)
    Kt = np.zeros((n_out, max(ns)), dtype=np.int32)
    for r, K in enumerate(rows):
        Kt[r, :len(K)] = K
    return np.array(xmins, dtype=np.int32), np.array(ns, dtype=np.int32), Kt


def _sums(img, n_out):
    """unclamped, unshifted sums of one pass along axis 1: img uint8 [R, n_in, C] -> int64 [R, n_out, C]"""
    xmin, n, K = coefficients(img.shape[1], n_out)
    out = np.empty((img.shape[0], n_out, img.shape[2]), dtype=np.int64)
    src = img.astype(np.int64)
    for xx in range(n_out):
        seg = src[:, xmin[xx]:xmin[xx] + n[xx], :]
        out[:, xx, :] = (1 << (PRECISION_BITS - 1)) + np.tensordot(seg, K[xx, :n[xx]].astype(np.int64), axes=([1], [0]))
    assert np.abs(out).max() < 2 ** 31  # the sums fit Pillow's int32
    return out


def _pass(img, n_out, saturated=None):
    s = _sums(img, n_out) >> PRECISION_BITS  # arithmetic shift
    if saturated is not None:
        saturated[0] += int((s < 0).sum())
        saturated[1] += int((s > 255).sum())
    return np.clip(s, 0, 255).astype(np.uint8)


def resize(img, hw, saturated=None):
    """img uint8 [H, W, 3] -> uint8 [h, w, 3].  `saturated`, a list [below, above], counts the sums the clamps caught."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = hw
    if w != img.shape[1]:
        img = _pass(img, w, saturated)
    if h != img.shape[0]:
        img = _pass(img.transpose(1, 0, 2), h, saturated).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


def normalisation_table(normalize=True):
    """float32 [3, 256]: what `_pil_to_normalised` makes of byte u in channel c (normalize=False: u / 255 only)"""
    t = np.arange(256, dtype=np.float32)[None, :].repeat(3, 0) / np.float32(255.0)
    if normalize:
        mean = np.array(IMAGENET_MEAN, dtype=np.float32)[:, None]
        std = np.array(IMAGENET_STD, dtype=np.float32)[:, None]
        t = (t - mean) / std
    return t.astype(np.float32)


def preprocess(img, hw, normalize=True):
    """float32 [3, h, w]"""
    r = resize(img, hw)
    t = normalisation_table(normalize)
    return np.stack([t[c][r[:, :, c]] for c in range(3)])
