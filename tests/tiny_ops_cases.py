"""What the Tiny RoMa operator tests share (test_cpu_tiny_ops.py, test_gpu_tiny_ops.py): the cases, and for every operator of
csrc/tiny.hip (plus roma_op_resize_bilinear and the correlation GEMM as TinyRoMa calls them)
  *_ref   the operator in float64, written from its definition in include/roma_hip.h and the comments of tiny.hip, on the f32
          values the device reads; it returns the result and the error bound of every output element;
  *_f32   the operator restated in numpy float32 in the kernel's order of operations, every product and sum rounded (no FMA;
          update_f32 alone has a fused form as well, see there).
Bounds are derived, not tuned.  U = 2^-24 is the unit roundoff of f32; every sum inside a bound is evaluated in float64.
Inputs come from numpy's PCG64, seeded by the case."""
import copy
import functools
import math

import numpy as np

U = 2.0 ** -24
F64 = np.float64


def gen(*seed):
    return np.random.Generator(np.random.PCG64([int(s) for s in seed]))


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def normal(g, *shape, std=1.0, mean=0.0):
    return f32(g.standard_normal(shape) * std + mean)


def ratio(got, want, bound):
    """max(|got - want| / bound): an exact result under a zero bound counts 0, anything else under a zero bound, and NaN, inf"""
    err = np.abs(np.asarray(got, dtype=F64) - np.asarray(want, dtype=F64))
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / np.broadcast_to(bound, err.shape)).max())


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# ================================================================================================ conv2d_nhwc
# (B, H, W, Cin, Cout, K, S, P)
CONV_CASES = [(2, 7, 9, 1, 4, 3, 1, 1),     # Cin = 1, the scalar path
              (1, 8, 8, 1, 24, 1, 1, 0),    # the skip1 form
              (2, 9, 7, 4, 8, 3, 2, 1),     # odd extents at stride 2
              (1, 10, 6, 8, 24, 3, 2, 1),   # even extents at stride 2
              (2, 5, 5, 24, 24, 3, 1, 0),   # 3x3 without padding
              (1, 6, 11, 6, 12, 3, 1, 1),   # Cin % 4 != 0 and Cin > 1
              (1, 4, 4, 128, 64, 1, 1, 0),  # wide 1x1
              (1, 6, 6, 64, 64, 3, 1, 1),   # ReLU + residual
              (3, 33, 17, 4, 4, 3, 1, 1)]   # more than one block of 256 threads
CONV_MISALIGNED = (2, 9, 7, 4, 8, 3, 2, 1)  # run once more with `in` one float off a 16-byte boundary
# Cout = 6, K = 5, stride 3, pad 2, and an empty output
CONV_REFUSALS = [(1, 6, 6, 4, 6, 3, 1, 1), (1, 6, 6, 4, 8, 5, 1, 1), (1, 6, 6, 4, 8, 3, 3, 1), (1, 6, 6, 4, 8, 3, 1, 2), (1, 1, 6, 4, 8, 3, 1, 0)]
CONV_FLAGS = [(b, r, s) for b in (1, 0) for r in (0, 1) for s in (0, 1)]  # (bias, relu, res)


def conv_out_size(H, W, K, S, P):
    return (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1


def conv_inputs(case):
    """x [B,H,W,Cin], w [K*K*Cin][Cout] (tap-major), bias [Cout], res [B,Ho,Wo,Cout]: zero-mean, so that about half of the
    pre-activations and half of the residuals are negative and ReLU(acc) + res differs from ReLU(acc + res)"""
    B, H, W, Cin, Cout, K, S, P = case
    Ho, Wo = conv_out_size(H, W, K, S, P)
    g = gen(11, *case)
    return (normal(g, B, H, W, Cin), normal(g, K * K * Cin, Cout, std=1.0 / math.sqrt(K * K * Cin)), normal(g, Cout, std=0.5),
            normal(g, B, max(Ho, 1), max(Wo, 1), Cout))


def _taps(xp, K, S, Ho, Wo):
    for ky in range(K):
        for kx in range(K):
            yield ky * K + kx, xp[:, ky:ky + S * (Ho - 1) + 1:S, kx:kx + S * (Wo - 1) + 1:S, :]


def conv_ref(x, w, bias, res, K, S, P, relu, extra_ops=0):
    """out = act(bias + sum over taps and channels) + res, and the bound (n + 3 + extra_ops) U (sum |x w| + |bias| + |res|) with
    n the number of products of that output that lie inside the image (ReLU is 1-Lipschitz: the bound passes through it)"""
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    Ho, Wo = conv_out_size(H, W, K, S, P)
    pad = ((0, 0), (P, P), (P, P), (0, 0))
    xp, inside = np.pad(x.astype(F64), pad), np.pad(np.ones((1, H, W, 1)), pad)
    w3 = w.astype(F64).reshape(K * K, Cin, Cout)
    acc, mag, n = np.zeros((B, Ho, Wo, Cout)), np.zeros((B, Ho, Wo, Cout)), np.zeros((1, Ho, Wo, 1))
    for t, p in _taps(xp, K, S, Ho, Wo):
        acc += p @ w3[t]
        mag += np.abs(p) @ np.abs(w3[t])
    for _, p in _taps(inside, K, S, Ho, Wo):
        n += p * Cin
    if bias is not None:
        acc += bias.astype(F64)
        mag += np.abs(bias.astype(F64))
    if relu:
        acc = np.maximum(acc, 0.0)
    if res is not None:
        acc += res.astype(F64)
        mag += np.abs(res.astype(F64))
    return acc, (n + 3 + extra_ops) * U * mag


def conv_f32(x, w, bias, res, K, S, P, relu):
    """acc = bias; for ky, kx, ci: acc += in * w; ReLU; + res (a tap outside the image adds an exact zero here, the kernel skips it)"""
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    Ho, Wo = conv_out_size(H, W, K, S, P)
    xp = np.pad(f32(x), ((0, 0), (P, P), (P, P), (0, 0)))
    w3 = f32(w).reshape(K * K, Cin, Cout)
    acc = np.zeros((B, Ho, Wo, Cout), dtype=np.float32) + (f32(bias) if bias is not None else np.float32(0))
    for t, p in _taps(xp, K, S, Ho, Wo):
        for ci in range(Cin):
            acc = acc + p[..., ci:ci + 1] * w3[t, ci]
    if relu:
        acc = np.maximum(acc, np.float32(0))
    if res is not None:
        acc = acc + f32(res)
    assert acc.dtype == np.float32
    return acc


# ================================================================================================ avgpool_nhwc
AVGPOOL_CASES = [(2, 8, 12, 1, 4), (1, 9, 14, 3, 4), (1, 7, 7, 5, 3), (1, 4, 4, 24, 4)]  # (B, H, W, C, k)
AVGPOOL_REFUSAL = (1, 3, 8, 2, 4)  # H < k


def avgpool_inputs(case):
    B, H, W, C, k = case
    return normal(gen(12, *case), B, H, W, C, mean=0.3)


def _windows(x, k):
    B, H, W, C = x.shape
    Ho, Wo = H // k, W // k
    return x[:, :Ho * k, :Wo * k].reshape(B, Ho, k, Wo, k, C)


def avgpool_ref(x, k):
    """AvgPool2d(k, k), floor: rows and columns beyond Ho k, Wo k are not read.  k^2 - 1 additions, the rounding of 1/k^2 and
    the product: (k^2 + 1) U sum|x| / k^2"""
    win = _windows(x.astype(F64), k)
    return win.sum(axis=(2, 4)) / (k * k), (k * k + 1) * U * np.abs(win).sum(axis=(2, 4)) / (k * k)


def avgpool_f32(x, k):
    win = _windows(f32(x), k)
    a = np.zeros(win[:, :, 0, :, 0].shape, dtype=np.float32)
    for dy in range(k):
        for dx in range(k):
            a = a + win[:, :, dy, :, dx]
    return a * (np.float32(1) / np.float32(k * k))


# ================================================================================================ gray_instnorm
INSTNORM_CASES = [(3, 5, 7, 3, 1e-5),    # 35 pixels for 1024 threads
                  (1, 32, 32, 1, 1e-5),  # exactly 1024 pixels
                  (2, 32, 40, 3, 1e-3),  # 1280 pixels: a ragged second trip
                  (1, 1, 1, 3, 1e-5)]    # one pixel: variance 0
INSTNORM_THREADS = 1024


def instnorm_inputs(case):
    """mean 0.5, std 0.2; the images of a batch differ in mean by 0.1, so an image normalised with its neighbour's statistics is
    off by half a standard deviation"""
    B, H, W, C, _ = case
    g = gen(13, *case[:4])
    return f32(normal(g, B, H, W, C, std=0.2, mean=0.5) + 0.1 * np.arange(B, dtype=np.float32).reshape(B, 1, 1, 1))


def instnorm_constant():
    """(2, 5, 7, 3) with the images 0.5 and 0.25 everywhere: the gray value, its sum over 35 pixels and the mean are exact in
    f32 however they are evaluated, so the output is exactly 0"""
    x = np.empty((2, 5, 7, 3), dtype=np.float32)
    x[0], x[1] = 0.5, 0.25
    return x


def instnorm_ref(x, eps):
    """InstanceNorm2d(1) (no affine, biased variance) of the channel mean.  Summation depth d = C + ceil(HW / 1024) + 10 (the
    channels, a thread's trips, the tree over 1024 threads); the bound is 4 d U (max|gray| inv_std + |out|) per pixel"""
    B, H, W, C = x.shape
    HW = H * W
    g = x.astype(F64).reshape(B, HW, C).sum(axis=2) / C
    mean = g.mean(axis=1, keepdims=True)
    var = ((g - mean) ** 2).mean(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(var + float(np.float32(eps)))
    out = (g - mean) * inv
    d = C + -(-HW // INSTNORM_THREADS) + 10
    bound = 4 * d * U * (np.abs(g).max(axis=1, keepdims=True) * inv + np.abs(out))
    return out.reshape(B, H, W, 1), bound.reshape(B, H, W, 1)


def instnorm_f32(x, eps):
    B, H, W, C = x.shape
    HW, T = H * W, INSTNORM_THREADS
    x = f32(x).reshape(B, HW, C)
    g = np.zeros((B, HW), dtype=np.float32)
    for c in range(C):
        g = g + x[:, :, c]
    g = g * (np.float32(1) / np.float32(C))

    def block_sum(v):  # a thread adds its pixels p, p + 1024, ...; then the tree 512, 256, ... 1
        trips = -(-HW // T)
        v = np.concatenate([v, np.zeros((B, trips * T - HW), dtype=np.float32)], axis=1).reshape(B, trips, T)
        red = np.zeros((B, T), dtype=np.float32)
        for t in range(trips):
            red = red + v[:, t]
        off = T // 2
        while off >= 1:
            red = red[:, :off] + red[:, off:2 * off]
            off //= 2
        return red  # [B, 1]

    mean = block_sum(g) / np.float32(HW)
    d = g - mean
    inv = np.float32(1) / np.sqrt(block_sum(d * d) / np.float32(HW) + np.float32(eps))
    out = (g - mean) * inv
    assert out.dtype == np.float32
    return out.reshape(B, H, W, 1)


# ================================================================================================ nchw_to_nhwc, add3
NCHW_CASES = [(2, 3, 5, 7), (1, 64, 3, 2)]  # (B, C, H, W)
ADD3_SIZES = [1, 255, 257, 70001]


def add3_inputs(n):
    g = gen(14, n)
    return normal(g, n), normal(g, n, std=3.0), normal(g, n, std=0.1)


# ================================================================================================ tiny_pos_embed
# (B, H1, W1, H0, W0, kind): "soft" scales the columns to the spread of the indices 0..15 so the soft part decides; "swamped"
# puts every column's maximum at a large index, whose logit then swamps the rest: the result is the grid point of the arg-max
POS_CASES = [(2, 4, 4, 3, 5, "soft"), (1, 8, 4, 4, 8, "plain"), (1, 12, 8, 2, 2, "swamped"), (2, 4, 8, 17, 16, "plain")]
POS_REFUSAL = (1, 6, 4, 2, 2)  # inference mode: H1 = 6 is no multiple of 4


def pos_ties(case):
    """per query 0, 1, 2: the positions that share the column's maximum.  (0, W1 + 1) ties a position on the 4x sub-grid with
    one off it."""
    _, H1, W1, _, _, kind = case
    n1 = H1 * W1
    if kind == "swamped":
        return [(n1 - 20, n1 - 3), (n1 - 30, n1 - 9, n1 - 1), (n1 - 5, n1 - 4)]
    return [(0, W1 + 1), (2, n1 // 2 + 1, n1 - 1), (W1 + 2, n1 - 2)]


def pos_inputs(case):
    """cv [B, H1*W1, H0*W0]"""
    B, H1, W1, H0, W0, kind = case
    n1, N0 = H1 * W1, H0 * W0
    g = gen(15, B, H1, W1, H0, W0)
    cv = normal(g, B, n1, N0, std=6.0 if kind == "soft" else 1.0)
    if kind == "swamped":
        j = g.integers(3 * n1 // 4, n1, size=(B, N0))
        top = cv.max(axis=1) + np.float32(0.5)
        np.put_along_axis(cv, j[:, None, :], top[:, None, :], axis=1)
    for q, tie in enumerate(pos_ties(case)):
        cv[:, list(tie), q] = cv[:, :, q].max(axis=1, keepdims=True) + np.float32(1)
    return cv


def pix_coords(n):
    return np.linspace(-1 + 1 / n, 1 - 1 / n, n)


@functools.lru_cache(maxsize=None)
def expf_ulp():
    """The allowance for expf, in ulp.  The ROCm installation carries no accuracy table of its device library, so the figure
    is the f32 restatement's own: the largest error of numpy's float32 exp against float64 over [-87.3, 0], the arguments a
    max-subtracted softmax can produce with a normal result, rounded up to a whole ulp (numpy's vectorised float32 exp is good
    to 2.52 ulp by its own account, so this is 3 where numpy takes that path and 1 where it calls the C library)."""
    x = np.linspace(-87.3, 0.0, 400001).astype(np.float32)
    e = np.exp(x)
    return int(math.ceil(float((np.abs(e.astype(F64) - np.exp(x.astype(F64))) / np.spacing(e).astype(F64)).max())))


def pos_embed_ref(cv, H1, W1, exact):
    """out [B, N0, 2] and its bound.  Inference: best = first arg-max of the f32 column (exact), P = softmax over the column at
    the 4x sub-grid (y-major) and float(best) - the index, as the kernel comment states -, out = sum P_k grid_lr[k] +
    P_last grid[best].  exact: softmax over all positions.  Outputs are convex combinations of coordinates in [-1, 1]:
    (n_terms + 16) 2U absolute, plus expf: a relative error e_k in every weight moves the output by sum P_k e_k (g_k - out),
    at most expf_ulp() 2U sum P_k |g_k - out|."""
    B, n1, N0 = cv.shape
    c = cv.astype(F64)
    gx, gy = np.tile(pix_coords(W1), H1), np.repeat(pix_coords(H1), W1)  # position j = y W1 + x
    if exact:
        logits = c
        X, Y = np.broadcast_to(gx[None, :, None], c.shape), np.broadcast_to(gy[None, :, None], c.shape)
    else:
        hl, wl = H1 // 4, W1 // 4
        best = np.argmax(cv, axis=1)  # first maximum
        lr = (4 * np.arange(hl)[:, None] * W1 + 4 * np.arange(wl)[None, :]).ravel()
        lx, ly = np.tile(np.linspace(-1 + 4 / W1, 1 - 4 / W1, wl), hl), np.repeat(np.linspace(-1 + 4 / H1, 1 - 4 / H1, hl), wl)
        logits = np.concatenate([c[:, lr, :], best[:, None, :].astype(F64)], axis=1)
        X = np.concatenate([np.broadcast_to(lx[None, :, None], (B, hl * wl, N0)), gx[best][:, None, :]], axis=1)
        Y = np.concatenate([np.broadcast_to(ly[None, :, None], (B, hl * wl, N0)), gy[best][:, None, :]], axis=1)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    out = np.stack([(p * X).sum(axis=1), (p * Y).sum(axis=1)], axis=-1)
    spread = np.stack([(p * np.abs(X - out[:, None, :, 0])).sum(axis=1), (p * np.abs(Y - out[:, None, :, 1])).sum(axis=1)], axis=-1)
    return out, (logits.shape[1] + 16) * 2 * U + expf_ulp() * 2 * U * spread


def _coord_f32(i, n):  # tiny_pix_coord
    return np.float32(-1) + (np.float32(2) * np.asarray(i, dtype=np.float32) + np.float32(1)) / np.float32(n)


def pos_embed_f32(cv, H1, W1, exact):
    cv = f32(cv)
    B, n1, N0 = cv.shape
    s, px, py = (np.zeros((B, N0), dtype=np.float32) for _ in range(3))
    if exact:
        m = cv.max(axis=1)
        for y in range(H1):
            for x in range(W1):
                e = np.exp(cv[:, y * W1 + x, :] - m)
                s, px, py = s + e, px + e * _coord_f32(x, W1), py + e * _coord_f32(y, H1)
    else:
        hl, wl = H1 // 4, W1 // 4
        best = np.argmax(cv, axis=1)
        extra = best.astype(np.float32)
        m = extra
        for y in range(hl):
            for x in range(wl):
                m = np.maximum(m, cv[:, 4 * y * W1 + 4 * x, :])
        for y in range(hl):
            gy = np.float32(-1) + (np.float32(4) * (np.float32(2) * np.float32(y) + np.float32(1))) / np.float32(H1)
            for x in range(wl):
                e = np.exp(cv[:, 4 * y * W1 + 4 * x, :] - m)
                s, px, py = s + e, px + e * (np.float32(-1) + (np.float32(4) * (np.float32(2) * np.float32(x) + np.float32(1))) / np.float32(W1)), py + e * gy
        el = np.exp(extra - m)
        s, px, py = s + el, px + el * _coord_f32(best % W1, W1), py + el * _coord_f32(best // W1, H1)
    out = np.stack([px / s, py / s], axis=-1)
    assert out.dtype == np.float32
    return out


# ================================================================================================ bilinear sampling (shared)
PAD = 3


def _bilinear(fp, iy, ix, extent):
    """fp [B, H + 2 PAD, W + 2 PAD, C] float64, padded by PAD; iy, ix [B, h, w] float64 source coordinates in un-padded pixels,
    clipped by the caller so that every tap lies inside the padding.  Returns the blend sum_t w_t f_t and its bound
      8 U sum_t |w_t f_t|  +  4 U extent max|f_a - f_b|
    The first term is the blend; the second covers the f32 source coordinate: three roundings of a value below 1.25 extent move
    it by less than 4 U extent, and the interpolant is continuous and piecewise linear with slopes |f_a - f_b| along either
    axis.  The taps a, b are the four of the cell; where the coordinate is within 4 U extent above an integer, the f32
    coordinate may fall into the cell before it (a flipped floor), so that cell's taps count too."""
    B = fp.shape[0]
    y0, x0 = np.floor(iy), np.floor(ix)
    ty, tx = iy - y0, ix - x0
    yi, xi = y0.astype(np.int64) + PAD, x0.astype(np.int64) + PAD
    b = np.arange(B).reshape(B, 1, 1)
    tol = 4 * U * extent
    val = mag = 0.0
    hi, lo = np.full(iy.shape + fp.shape[-1:], -np.inf), np.full(iy.shape + fp.shape[-1:], np.inf)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            f = fp[b, yi + dy, xi + dx]  # [B, h, w, C]
            ok = ((ty < tol) if dy < 0 else np.ones_like(ty, dtype=bool)) & ((tx < tol) if dx < 0 else np.ones_like(tx, dtype=bool))
            hi, lo = np.where(ok[..., None], np.maximum(hi, f), hi), np.where(ok[..., None], np.minimum(lo, f), lo)
            if dy >= 0 and dx >= 0:
                wt = ((ty if dy else 1 - ty) * (tx if dx else 1 - tx))[..., None]
                val, mag = val + wt * f, mag + np.abs(wt * f)
    return val, 8 * U * mag + 4 * U * extent * (hi - lo)


# ================================================================================================ tiny_matcher_input
MATCHER_CASES = [(2, 3, 5, 4, 6, 8, 24, 2), (1, 4, 4, 5, 3, 24, 64, 3), (1, 2, 2, 1, 1, 4, 10, 2)]  # (B, H, W, H1, W1, C, Cp, wc)
MATCHER_REFUSAL = (1, 2, 2, 3, 3, 4, 9, 2)  # Cp < 2 C + 2


def matcher_inputs(case):
    """f0 [B,H,W,C], f1 [B,H1,W1,C], warp [B,H,W,wc].  The warp holds, in random order: pixel centres, exact -1 and +1, samples
    half a pixel outside each border, +-1e30 and +-inf, and uniform coordinates in [-1.5, 1.5] for the rest (where there are
    fewer pixels than special samples, a random choice of them)."""
    B, H, W, H1, W1, C, Cp, wc = case
    g = gen(16, *case)
    f0, f1 = normal(g, B, H, W, C), normal(g, B, H1, W1, C)
    n = B * H * W
    cx, cy = lambda i: -1 + (2 * i + 1) / W1, lambda i: -1 + (2 * i + 1) / H1  # noqa: E731
    inf = math.inf
    special = [(cx(0), cy(H1 - 1)), (cx(W1 // 2), cy(H1 // 2)), (-1, -1), (1, 1), (-1, 1),
               (-1 - 1 / W1, 0.3), (1 + 1 / W1, -0.2), (0.1, -1 - 1 / H1), (-0.4, 1 + 1 / H1),
               (1e30, 0.1), (0.2, -1e30), (inf, 0.0), (0.0, -inf), (-inf, inf)]
    xy = g.uniform(-1.5, 1.5, size=(n, 2))
    if n >= len(special):
        xy[:len(special)] = special
    else:
        xy[:] = np.asarray(special)[g.choice(len(special), size=n, replace=False)]
    warp = g.uniform(-1.0, 1.0, size=(n, wc))
    warp[:, :2] = xy[g.permutation(n)]
    return f0, f1, f32(warp).reshape(B, H, W, wc)


def matcher_sample_ref(f1, warp):
    """grid_sample(f1, warp[..., 0:2]) (bilinear, zeros padding, align_corners=False) [B,H,W,C] and its bound.  Coordinates
    beyond the image by more than a pixel sample zeros, so clipping them to two pixels outside changes nothing and keeps
    +-1e30 and +-inf finite (the kernel clamps at +-1e6 for the same end)."""
    B, H1, W1, C = f1.shape
    fp = np.pad(f1.astype(F64), ((0, 0), (PAD, PAD), (PAD, PAD), (0, 0)))
    with np.errstate(invalid="ignore", over="ignore"):
        ix = np.clip(((warp[..., 0].astype(F64) + 1) * W1 - 1) / 2, -2.0, W1 + 1.0)
        iy = np.clip(((warp[..., 1].astype(F64) + 1) * H1 - 1) / 2, -2.0, H1 + 1.0)
    return _bilinear(fp, iy, ix, max(H1, W1))


def matcher_sample_f32(f1, warp):
    f1, warp = f32(f1), f32(warp)
    B, H1, W1, C = f1.shape
    one, half, lim = np.float32(1), np.float32(0.5), np.float32(1.0e6)
    with np.errstate(invalid="ignore", over="ignore"):
        ix = ((warp[..., 0] + one) * np.float32(W1) - one) * half
        iy = ((warp[..., 1] + one) * np.float32(H1) - one) * half
    ix, iy = np.minimum(np.maximum(ix, -lim), lim), np.minimum(np.maximum(iy, -lim), lim)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    tx, ty = ix - fx0, iy - fy0
    wgt = [(one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty]
    b = np.arange(B).reshape(B, 1, 1)
    v = np.zeros(warp.shape[:3] + (C,), dtype=np.float32)
    for t in range(4):
        yy, xx = y0 + (t >> 1), x0 + (t & 1)
        ok = (yy >= 0) & (yy < H1) & (xx >= 0) & (xx < W1)
        f = f1[b, np.clip(yy, 0, H1 - 1), np.clip(xx, 0, W1 - 1)]
        v = np.where(ok[..., None], v + wgt[t][..., None] * f, v)
    assert v.dtype == np.float32
    return v


def matcher_assemble(f0, sampled, warp, Cp):
    """d = [f0 | sampled | warp[..., 0:2] | 0 ...] as f32"""
    B, H, W, C = f0.shape
    d = np.zeros((B, H, W, Cp), dtype=np.float32)
    d[..., :C], d[..., C:2 * C], d[..., 2 * C:2 * C + 2] = f0, sampled, warp[..., :2]
    return d


# ================================================================================================ tiny_update
UPDATE_CASES = [(nb, ldd, npix) for nb in (2, 3) for ldd in (3, 4) for npix in (1, 255, 513)]  # (base_channels, ldd, npix)
UPDATE_REFUSALS = [(4, 4, 8), (2, 2, 8)]
UPDATE_SCALE = (2.0 / 37, 2.0 / 21)  # (sx, sy): 2 / W1, 2 / H1 of an image, inexact in f32


def update_inputs(case):
    """base [npix, nb], delta [npix, ldd]; a fourth delta column is NaN: it must not be read"""
    nb, ldd, npix = case
    g = gen(17, *case)
    base, delta = normal(g, npix, nb), normal(g, npix, ldd, std=4.0)
    if ldd > 3:
        delta[:, 3:] = np.nan
    return base, delta


def _update_terms(base, delta, dt):
    npix, nb = base.shape
    b = np.zeros((npix, 3), dtype=dt)
    b[:, :nb] = base
    s = np.array([np.float32(UPDATE_SCALE[0]), np.float32(UPDATE_SCALE[1]), 1.0], dtype=dt)  # the scales as the device gets them
    return b, delta[:, :3].astype(dt), s


def update_ref(base, delta):
    """out[p, 0:3] = base (missing channel = 0) + delta[p, 0:3] * (sx, sy, 1): 2U (|base| + |delta s|), fused or not"""
    b, d, s = _update_terms(base, delta, F64)
    return b + d * s, 2 * U * (np.abs(b) + np.abs(d * s))


def update_f32(base, delta, fused=True):
    """fused: one rounding of base + delta s, what a contracting compiler makes of the kernel's line (the product of two f32 is
    exact in float64).  Unfused, the product's rounding comes on top and the error can reach U (|base| + 2 |delta s|): past half
    of the bound, never past the bound."""
    if fused:
        b, d, s = _update_terms(base, delta, F64)
        return (b + d * s).astype(np.float32)
    b, d, s = _update_terms(base, delta, np.float32)
    return b + d * s


# ================================================================================================ tiny_final
FINAL_CASES = [(2, 3, 5), (1, 1, 1), (1, 17, 31)]  # (B, H, W)
FINAL_LOGITS = [0.0, 20.0, -20.0, 90.0, -90.0, math.inf, -math.inf]
FINAL_GRID_BOUND, FINAL_CERT_BOUND = 4 * U, 8 * U


def final_inputs(case):
    """matches [B,H,W,3]: flow (two channels) and certainty logits, the special logits first where they fit.  The other
    logits stay below 10 in size: between 16.6 and 17.3 sigmoid lies within U of 1 and the f32 sum 1 + e^-z already rounds to 1
    where the float64 value still rounds to 1 - U, which is no fault of a kernel."""
    B, H, W = case
    m = normal(gen(18, *case), B * H * W, 3, std=5.0)
    m[:, 2] = np.clip(m[:, 2] * np.float32(0.4), -10, 10)
    k = min(len(FINAL_LOGITS), B * H * W)
    m[:k, 2] = FINAL_LOGITS[:k]
    return m.reshape(B, H, W, 3)


def final_special_logits():
    """[1,1,7,3]: every special logit, whatever the cases hold"""
    m = normal(gen(18), 1, 1, len(FINAL_LOGITS), 3)
    m[0, 0, :, 2] = FINAL_LOGITS
    return m


def final_ref(m):
    """warp = (grid_x, grid_y, flow_x, flow_y) with grid = linspace(-1 + 1/n, 1 - 1/n, n); certainty = sigmoid(logit)"""
    B, H, W, _ = m.shape
    warp = np.empty((B, H, W, 4))
    warp[..., 0], warp[..., 1] = pix_coords(W)[None, None, :], pix_coords(H)[None, :, None]
    warp[..., 2:] = m[..., :2]
    with np.errstate(over="ignore"):
        cert = 1.0 / (1.0 + np.exp(-m[..., 2].astype(F64)))
    return warp, cert


def final_f32(m):
    m = f32(m)
    B, H, W, _ = m.shape
    warp = np.empty((B, H, W, 4), dtype=np.float32)
    warp[..., 0], warp[..., 1] = _coord_f32(np.arange(W), W)[None, None, :], _coord_f32(np.arange(H), H)[None, :, None]
    warp[..., 2:] = m[..., :2]
    z = m[..., 2]
    with np.errstate(over="ignore"):
        cert = np.where(z < np.float32(-87), np.exp(np.minimum(z, np.float32(0))), np.float32(1) / (np.float32(1) + np.exp(-z)))
    assert cert.dtype == np.float32
    return warp, cert


def check_final_cert(got, m):
    """no NaN, within the bound, and exactly 0 or 1 only where the float64 sigmoid rounds there in f32"""
    _, want = final_ref(m)
    got = np.asarray(got, dtype=np.float32)
    assert not np.isnan(got).any()
    with np.errstate(under="ignore"):
        w32 = want.astype(np.float32)
    for edge in (0.0, 1.0):
        assert not ((got == edge) & (w32 != edge)).any(), (edge, m[..., 2][(got == edge) & (w32 != edge)])
    return ratio(got, want, FINAL_CERT_BOUND)


# ================================================================================================ resize_bilinear
RESIZE_CASES = [(2, 5, 9, 10, 18, 3),    # up by two, not square
                (1, 9, 5, 4, 7, 3),      # down in H, up in W
                (1, 4, 6, 8, 12, 64),    # the backbone's feature maps
                (2, 37, 50, 32, 32, 3),  # the resize to a multiple of 32
                (1, 3, 3, 3, 3, 24)]     # identity: bit-exact
RESIZE_IDENTITY = RESIZE_CASES[-1]  # (B, Hin, Win, Hout, Wout, nc)


def resize_inputs(case):
    B, Hin, Win, _, _, nc = case
    return normal(gen(19, *case), B, Hin, Win, nc)


def resize_ref(x, Hout, Wout, swap_scales=False):
    """F.interpolate(bilinear, align_corners=False): src = max(in/out (dst + 0.5) - 0.5, 0), taps i0 = floor(src) and
    min(i0 + 1, in - 1) - edge padding says the same.  swap_scales: the wrong operator that takes H's scale for W and W's
    for H (coordinates clipped to the image), to show that the cases tell the two apart."""
    B, Hin, Win, nc = x.shape
    fp = np.pad(x.astype(F64), ((0, 0), (PAD, PAD), (PAD, PAD), (0, 0)), mode="edge")
    sh, sw = (Win / Wout, Hin / Hout) if swap_scales else (Hin / Hout, Win / Wout)
    sy = np.clip(sh * (np.arange(Hout) + 0.5) - 0.5, 0.0, Hin - 0.5)
    sx = np.clip(sw * (np.arange(Wout) + 0.5) - 0.5, 0.0, Win - 0.5)
    iy, ix = np.broadcast_to(sy[None, :, None], (B, Hout, Wout)), np.broadcast_to(sx[None, None, :], (B, Hout, Wout))
    return _bilinear(fp, iy, ix, max(Hin, Win))


def resize_f32(x, Hout, Wout):
    x = f32(x)
    B, Hin, Win, nc = x.shape
    one, half = np.float32(1), np.float32(0.5)

    def src(n_out, n_in):
        s = np.maximum((np.float32(n_in) / np.float32(n_out)) * (np.arange(n_out, dtype=np.float32) + half) - half, np.float32(0))
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0.astype(np.float32)

    y0, y1, ly = src(Hout, Hin)
    x0, x1, lx = src(Wout, Win)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    v00, v01, v10, v11 = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    out = (one - ly) * ((one - lx) * v00 + lx * v01) + ly * ((one - lx) * v10 + lx * v11)
    assert out.dtype == np.float32
    return out


# ================================================================================================ correlation volume
CORR_CASES = [(2, 32, 30, 64), (1, 16, 48, 64), (3, 20, 12, 24)]  # (B, n1, n0, C)


def corr_inputs(case):
    """f1 [B, n1, C] (image B), f0 [B, n0, C] (image A): the two differ in scale and in mean, so swapped operands show"""
    B, n1, n0, C = case
    g = gen(20, *case)
    return normal(g, B, n1, C, std=2.0, mean=0.5), normal(g, B, n0, C, std=0.5, mean=-0.25)


def corr_alpha(C):
    return float(np.float32(1.0 / math.sqrt(C)))  # the f32 the GEMM receives


def corr_ref(f1, f0):
    """cv[b, j, i] = <f1[b, j], f0[b, i]> alpha: C products and the scaling, (C + 1 + 3) U sum|f1 f0| alpha"""
    C = f1.shape[-1]
    a = corr_alpha(C)
    acc = np.einsum("bjc,bic->bji", f1.astype(F64), f0.astype(F64))
    mag = np.einsum("bjc,bic->bji", np.abs(f1.astype(F64)), np.abs(f0.astype(F64)))
    return acc * a, (C + 1 + 3) * U * mag * a


def corr_f32(f1, f0):
    f1, f0 = f32(f1), f32(f0)
    acc = np.zeros(f1.shape[:2] + f0.shape[1:2], dtype=np.float32)
    for c in range(f1.shape[-1]):
        acc = acc + f1[:, :, None, c] * f0[:, None, :, c]
    return acc * np.float32(corr_alpha(f1.shape[-1]))


# ================================================================================================ the stack compiler
def _seed_module(m, seed):
    import torch
    g = gen(21, seed)
    with torch.no_grad():
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            leaf = name.rsplit(".", 1)[-1]
            if leaf == "num_batches_tracked":
                continue
            if leaf == "running_var":
                v = g.uniform(0.5, 2.0, size=tuple(t.shape))
            elif leaf == "running_mean":
                v = g.standard_normal(tuple(t.shape)) * 0.5
            elif t.dim() == 1 and leaf == "weight":  # BatchNorm scale, either sign
                v = g.uniform(0.5, 1.5, size=tuple(t.shape)) * g.choice([-1.0, 1.0], size=tuple(t.shape))
            elif t.dim() == 1:
                v = g.standard_normal(tuple(t.shape)) * 0.5
            else:
                v = g.standard_normal(tuple(t.shape)) / math.sqrt(t[0].numel())
            t.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    return m.train(False)


def stacks():
    """name -> (module, input shape [B,H,W,C]); seeded weights, running statistics away from (0, 1)"""
    import torch
    nn = torch.nn
    a = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=True), nn.BatchNorm2d(8, affine=True, eps=1e-3), nn.ReLU(),
                      nn.Conv2d(8, 12, 1, bias=False), nn.BatchNorm2d(12, affine=False), nn.Conv2d(12, 4, 1))
    b = nn.Sequential(nn.AvgPool2d(4, 4), nn.Conv2d(1, 24, 1))
    c = nn.Sequential(nn.Identity(),
                      nn.Sequential(nn.Conv2d(4, 8, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(8, affine=False), nn.ReLU()),
                      nn.Sequential(nn.Sequential(nn.Conv2d(8, 8, 3, stride=2, padding=1), nn.Identity(), nn.BatchNorm2d(8), nn.ReLU()),
                                    nn.Identity()))
    return {"a": (_seed_module(a, 1), (2, 9, 12, 3)), "b": (_seed_module(b, 2), (1, 15, 18, 1)), "c": (_seed_module(c, 3), (1, 16, 20, 4))}


def refused_stacks():
    """name -> module that _compile_stack must refuse with NotImplementedError"""
    import torch
    nn = torch.nn
    seq = nn.Sequential
    return {"dilation 2": seq(nn.Conv2d(4, 8, 3, padding=1, dilation=2)), "groups 2": seq(nn.Conv2d(4, 8, 3, padding=1, groups=2)),
            "5x5": seq(nn.Conv2d(4, 8, 5, padding=1)), "reflect": seq(nn.Conv2d(4, 8, 3, padding=1, padding_mode="reflect")),
            "AvgPool2d(3, 2)": seq(nn.AvgPool2d(3, 2)), "ReLU first": seq(nn.ReLU(), nn.Conv2d(4, 8, 1)),
            "BatchNorm after ReLU": seq(nn.Conv2d(4, 8, 1), nn.ReLU(), nn.BatchNorm2d(8)),
            "ceil_mode": seq(nn.AvgPool2d(4, 4, ceil_mode=True), nn.Conv2d(1, 24, 1)),
            "pool padding": seq(nn.AvgPool2d(4, 4, padding=1))}


def stack_input(shape, seed):
    return normal(gen(22, seed, *shape), *shape)


def _leaf_modules(m):
    kids = list(m.children())
    if not kids:
        yield m
    for k in kids:
        yield from _leaf_modules(k)


def stack_layers(m):
    """the torch module cut into one float64 module per compiled op: a convolution with the BatchNorm2d / ReLU behind it, or a pool"""
    import torch
    nn = torch.nn
    groups = []
    for leaf in _leaf_modules(m):
        if isinstance(leaf, nn.Identity):
            continue
        if isinstance(leaf, (nn.Conv2d, nn.AvgPool2d)):
            groups.append([])
        groups[-1].append(copy.deepcopy(leaf))
    return [nn.Sequential(*g).double().train(False) for g in groups]


def check_stack(m, ops, x, run_op):
    """Layer by layer: run_op(op, x) -> what the compiled op makes of x [B,H,W,C] f32 (a device operator, or the float64
    reference), held against the torch layer in float64 on the same x, so every layer answers for itself alone.  The bound is
    the operator's, with one more operation for the rounding of the folded weights and bias to f32.  Returns the worst ratio."""
    import torch
    layers = stack_layers(m)
    assert len(layers) == len(ops), (len(layers), len(ops))
    worst = 0.0
    for layer, o in zip(layers, ops):
        with torch.no_grad():
            want = layer(torch.from_numpy(x).double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
        got = run_op(o, x)
        if o["op"] == "conv":
            w, b = o["w"].cpu().numpy(), o["b"].cpu().numpy()
            assert w.dtype == np.float32 and w.shape == (o["k"] * o["k"] * o["cin"], o["cout"]) and b.shape == (o["cout"],)
            _, bound = conv_ref(x, w, b, None, o["k"], o["s"], o["p"], o["relu"], extra_ops=1)
        else:
            _, bound = avgpool_ref(x, o["k"])
        assert got.shape == want.shape, (got.shape, want.shape)
        worst = max(worst, ratio(got, want, bound))
        x = f32(got)
    return worst


def ref_run_op(o, x):
    """a compiled op evaluated with the float64 references"""
    if o["op"] == "conv":
        return conv_ref(x, o["w"].cpu().numpy(), o["b"].cpu().numpy(), None, o["k"], o["s"], o["p"], o["relu"])[0]
    return avgpool_ref(x, o["k"])[0]
