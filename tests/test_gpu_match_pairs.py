"""Cached per-image features: `match_pairs(encode_images(X), pairs)` must equal `match(X[pairs[:, 0]], X[pairs[:, 1]])` BIT FOR
BIT on the same handle with the same options - every kernel of match() gives per-row results that do not depend on the batch
(test_gpu_match.py::test_stream_split_*), and the encoded route runs the same kernels on the same rows: the encoders and proj
heads once per image, a gather kernel in place of the proj head, everything behind it unchanged."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

AMP = {"f32": (torch.float32, None), "bf16": (torch.bfloat16, None), "f16": (torch.float16, None),
       "mixed": (torch.bfloat16, torch.float16)}
ITEMSIZE = {"f32": 4, "bf16": 2, "f16": 2, "mixed": 2}


@pytest.fixture(scope="module")
def matchers(built_lib, weights0):
    """One matcher per (mode, coarse, upsample, max_batch), shared by the tests of this module."""
    from roma_amd import roma_model
    sd, dsd = weights0
    cache = {}

    def get(mode, coarse=(112, 112), up=(168, 168), max_batch=2):
        key = (mode, coarse, up, max_batch)
        if key not in cache:
            amp, dec = AMP[mode]
            cache[key] = roma_model(coarse, True, device="cuda:0", weights=sd, dinov2_weights=dsd, amp_dtype=amp, decoder_dtype=dec,
                                    symmetric=True, upsample_res=up, max_batch=max_batch)
        m = cache[key]
        m.symmetric, m.upsample_preds, m.dual_stream = True, True, True
        return m
    yield get
    cache.clear()


_IMAGES = {}


def _images(n, coarse, up, seed=11):
    """n coarse images and their high-resolution versions (roma_amd.synthetic), computed once per shape"""
    from roma_amd import synthetic
    key = (n, coarse, up, seed)
    if key not in _IMAGES:
        d = synthetic.make_inputs(n, coarse, up, seed=seed)
        _IMAGES[key] = (d["im_A"].cuda(), d["im_A_high_res"].cuda())
    return _IMAGES[key]


def _match(m, x, xh, pairs):
    ia, ib = [p[0] for p in pairs], [p[1] for p in pairs]
    if not m.upsample_preds:
        return m.match(x[ia], x[ib])
    return m.match(x[ia], x[ib], im_A_high_res=xh[ia], im_B_high_res=xh[ib])


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _diff(a, b):
    return float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_equal_shapes_exact(matchers, mode):
    """N = 4 images, 2 pairs on a max_batch = 2 handle: the encoders see 4 images on both routes."""
    m = matchers(mode)
    x, xh = _images(4, (112, 112), (168, 168))
    pairs = [(2, 0), (1, 3)]
    enc = m.encode_images(x, xh)
    for dual in (False, True):
        m.dual_stream = dual
        ref = _match(m, x, xh, pairs)
        got = m.match_pairs(enc, pairs)
        assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape
        assert _same(got, ref), (mode, dual, _diff(got, ref))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_reuse_and_odd_n_exact(matchers, mode):
    """N = 3 (an odd encoder batch), 4 pairs on a max_batch = 3 handle: chunks of 3 + 1; image 0 is query twice, image 2 is
    support and query in one chunk, and (2, 0) reverses (0, 2).  match() chunks its 4 pairs the same way."""
    m = matchers(mode, max_batch=3)
    x, xh = _images(3, (112, 112), (168, 168), seed=12)
    pairs = [(0, 1), (0, 2), (1, 2), (2, 0)]
    enc = m.encode_images(x, xh)
    ref = _match(m, x, xh, pairs)
    got = m.match_pairs(enc, np.asarray(pairs, dtype=np.int64))
    print("reuse / odd N", mode, _diff(got, ref))
    assert _same(got, ref), (mode, _diff(got, ref))


def test_odd_maps_exact(matchers):
    """(126, 154) -> (182, 198): a 9 x 11 token grid, feature grids that are no multiples of 8, slabs with odd hw."""
    m = matchers("f32", (126, 154), (182, 198), 1)
    x, xh = _images(2, (126, 154), (182, 198), seed=13)
    enc = m.encode_images(x, xh)
    ref = _match(m, x, xh, [(1, 0)])
    got = m.match_pairs(enc, [(1, 0)])
    assert _same(got, ref), _diff(got, ref)


def test_benchmark_geometry_exact(matchers):
    """560 -> 864, mixed precision, two streams: the ring kernels and the 1601-token attention exist only at this size.  Four
    packs of 120 MB stay below 2^31 bytes, so the same four packs are then addressed as images 18 .. 21 of a 22-pack buffer
    (2.6 GB): the gather's pack offsets pass 2^31 there."""
    import dataclasses
    from roma_amd.encoded import pack_layout
    m = matchers("mixed", (560, 560), (864, 864), 2)
    x, xh = _images(4, (560, 560), (864, 864), seed=14)
    pack = pack_layout((560, 560), (864, 864), 2)["total"]
    assert m.encoded_bytes() == pack and 2 ** 31 < 18 * pack
    big = torch.empty(22 * pack, dtype=torch.uint8, device="cuda:0")
    enc = m.encode_images(x, xh, out=big[18 * pack:])
    pairs = [(3, 1), (0, 2)]
    ref = _match(m, x, xh, pairs)
    got = m.match_pairs(enc, pairs)
    assert _same(got, ref), _diff(got, ref)
    enc22 = dataclasses.replace(enc, feats=big, n=22)
    got = m.match_pairs(enc22, [(21, 19), (18, 20)])
    assert _same(got, ref), _diff(got, ref)


def test_options(matchers):
    """symmetric = False, and upsample_preds = False on packs with and without the upsample part."""
    m = matchers("f32")
    x, xh = _images(4, (112, 112), (168, 168))
    pairs = [(2, 0), (1, 3)]
    enc_full = m.encode_images(x, xh)
    enc_coarse = m.encode_images(x)
    assert enc_full.has_upsample and not enc_coarse.has_upsample
    m.symmetric = False
    ref = _match(m, x, xh, pairs)
    got = m.match_pairs(enc_full, pairs)
    assert got[0].shape == (2, 168, 168, 4) and _same(got, ref), _diff(got, ref)
    m.symmetric, m.upsample_preds = True, False
    ref = _match(m, x, xh, pairs)
    for enc in (enc_coarse, enc_full):
        got = m.match_pairs(enc, pairs)
        assert got[0].shape == (2, 112, 224, 4) and _same(got, ref), _diff(got, ref)
    m.upsample_preds = True
    with pytest.raises(ValueError, match="coarse-only"):
        m.match_pairs(enc_coarse, pairs)
    # default pair list: all i < j, chunked 2 + 2 + 2
    from roma_amd.encoded import all_pairs
    got = m.match_pairs(enc_full)
    ref = _match(m, x, xh, all_pairs(4))
    assert got[0].shape[0] == 6 and _same(got, ref), _diff(got, ref)


def test_errors_leave_the_handle_usable(matchers):
    m = matchers("f32")
    other = matchers("f32", (126, 154), (182, 198), 1)
    x, xh = _images(4, (112, 112), (168, 168))
    xo, xoh = _images(2, (126, 154), (182, 198), seed=13)
    pairs = [(2, 0), (1, 3)]
    enc = m.encode_images(x, xh)
    enc_other = other.encode_images(xo, xoh)
    for bad in ([(0, -1)], [(4, 0)], [(0, 1), (1, 4)]):
        with pytest.raises(ValueError, match="outside"):
            m.match_pairs(enc, bad)
    with pytest.raises(ValueError, match="configuration"):
        m.match_pairs(enc_other, [(1, 0)])
    with pytest.raises(ValueError):
        m.match_pairs(enc, np.zeros((0, 2), dtype=np.int64))
    # the C entry points refuse the same things themselves: non-zero, roma_last_error set, nothing launched
    lib, h = m._lib, m._handle
    pack = m.encoded_bytes()
    assert pack == enc.pack_bytes and enc.feats.numel() == 4 * pack
    warp = torch.empty((2, 168, 336, 4), device="cuda:0")
    cert = torch.empty((2, 168, 336), device="cuda:0")
    ip = C.POINTER(C.c_int)

    def raw(P, nbytes, ia, ib):
        a, b = np.asarray(ia, dtype=np.int32), np.asarray(ib, dtype=np.int32)
        return lib.roma_match_encoded(h, P, C.c_void_p(enc.feats.data_ptr()), nbytes, 4, a.ctypes.data_as(ip), b.ctypes.data_as(ip),
                                      C.c_void_p(warp.data_ptr()), C.c_void_p(cert.data_ptr()), None)
    torch.cuda.synchronize()
    assert raw(2, 4 * pack - 256, [2, 1], [0, 3]) != 0 and b"feats_bytes" in lib.roma_last_error()
    assert raw(3, 4 * pack, [2, 1, 0], [0, 3, 1]) != 0 and b"max_batch" in lib.roma_last_error()
    assert raw(2, 4 * pack, [2, 4], [0, 3]) != 0 and b"outside" in lib.roma_last_error()
    assert raw(2, 4 * pack, [2, 1], [-1, 3]) != 0 and b"outside" in lib.roma_last_error()
    assert lib.roma_encode(h, 4, C.c_void_p(x.data_ptr()), C.c_void_p(xh.data_ptr()), C.c_void_p(enc.feats.data_ptr()), 4 * pack + 16,
                           None) != 0 and b"feats_bytes" in lib.roma_last_error()
    # a valid call afterwards still gives the exact result
    ref = _match(m, x, xh, pairs)
    got = m.match_pairs(enc, pairs)
    assert _same(got, ref), _diff(got, ref)


def test_cache_buffer_bounds_and_size(matchers):
    """The packs live inside a larger tensor whose bytes on both sides are all ones (NaN in every float format): encode_images
    and match_pairs leave them untouched, and roma_encoded_bytes is the total of the Python layout."""
    from roma_amd.encoded import pack_layout
    for mode, n in (("f32", 3), ("bf16", 3)):
        m = matchers(mode, max_batch=3)
        x, xh = _images(3, (112, 112), (168, 168), seed=12)
        pack = m.encoded_bytes()
        assert pack == pack_layout((112, 112), (168, 168), ITEMSIZE[mode])["total"]
        pad = 4096
        big = torch.full((pad + n * pack + pad,), 0xFF, dtype=torch.uint8, device="cuda:0")
        enc = m.encode_images(x, xh, out=big[pad:pad + n * pack])
        got = m.match_pairs(enc, [(0, 1), (2, 0)])
        torch.cuda.synchronize()
        assert bool((big[:pad] == 0xFF).all()) and bool((big[pad + n * pack:] == 0xFF).all())
        assert enc.feats.data_ptr() == big.data_ptr() + pad
        assert _same(got, _match(m, x, xh, [(0, 1), (2, 0)]))


def test_match_image_set_equals_match_images(matchers):
    """Three decoded images of different sizes (crops and resizes of the golden pair) -> one preprocess call, one encode, pairs."""
    from PIL import Image
    m = matchers("f32")
    a = Image.open(os.path.join(GOLDEN, "pair_A.png")).convert("RGB")
    b = Image.open(os.path.join(GOLDEN, "pair_B.png")).convert("RGB")
    w, h = a.size
    ims = [a, b.resize((max(w // 2, 32), max(h * 3 // 4, 32)), resample=Image.BILINEAR), a.crop((w // 8, h // 8, w - w // 7, h - h // 5))]
    assert len({im.size for im in ims}) == 3
    warp, cert, pairs = m.match_image_set(ims)
    assert pairs == [(0, 1), (0, 2), (1, 2)] and all(isinstance(p, tuple) for p in pairs)
    ref = m.match_images([ims[i] for i, _ in pairs], [ims[j] for _, j in pairs])
    assert _same((warp, cert), ref), _diff((warp, cert), ref)
    warp2, cert2, pairs2 = m.match_image_set(ims, [(2, 1)])
    ref2 = m.match_images([ims[2]], [ims[1]])
    assert pairs2 == [(2, 1)] and _same((warp2, cert2), ref2)
