"""roma_amd.preprocess_images / RegressionMatcher.match_images on the GPU against the host path they replace
(matcher._pil_to_normalised: PIL bicubic resize, / 255, mean / std).  Every comparison is an equality of bits: no tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import preprocess_cases as pc

pytestmark = pytest.mark.gpu

CASE_IDS = [c[0] for c in pc.cases()]
BATCH_TARGETS = ((56, 70), (84, 98))


def same_bits(got, want):
    """torch.equal on the bit patterns (so that -0.0 / +0.0 or a NaN could not hide a difference)"""
    want = torch.as_tensor(np.ascontiguousarray(want)) if not isinstance(want, torch.Tensor) else want
    got = got.detach().cpu().contiguous()
    return got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def batch_reference():
    """[target][case] float32 [3, h, w]: every case image through the host path, for both batch targets; computed once"""
    return tuple(tuple(pc.reference(img, hw, True) for _, img, _ in pc.cases()) for hw in BATCH_TARGETS)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "div255"])
@pytest.mark.parametrize("case", pc.cases(), ids=CASE_IDS)
def test_every_case_equals_the_host_path_bit_for_bit(built_lib, case, normalize):
    from PIL import Image
    import roma_amd
    from roma_amd.matcher import _pil_to_normalised
    _, img, hw = case
    out = roma_amd.preprocess_images([img], hw, normalize=normalize, device="cuda:0")
    assert out.is_cuda and tuple(out.shape) == (1, 3) + hw
    want = _pil_to_normalised(Image.fromarray(img), hw) if normalize else torch.as_tensor(pc.reference(img, hw, False))
    assert same_bits(out[0], want), f"{int((out[0].cpu() != want).sum())} of {want.numel()} values differ"


def test_mixed_size_batch_two_targets_is_order_and_batch_independent(built_lib):
    import roma_amd
    imgs = [img for _, img, _ in pc.cases()]
    ref = batch_reference()
    outs = roma_amd.preprocess_images(imgs, BATCH_TARGETS, device="cuda:0")
    assert isinstance(outs, tuple) and len(outs) == 2
    for t, hw in enumerate(BATCH_TARGETS):
        assert tuple(outs[t].shape) == (len(imgs), 3) + hw
        for i in range(len(imgs)):
            assert same_bits(outs[t][i], ref[t][i]), (hw, CASE_IDS[i])
    # each image alone
    for i, img in enumerate(imgs):
        alone = roma_amd.preprocess_images([img], BATCH_TARGETS, device="cuda:0")
        for t in range(2):
            assert same_bits(alone[t][0], outs[t][i].cpu()), (BATCH_TARGETS[t], CASE_IDS[i])
    # the same batch in permuted order, and a second run
    perm = np.random.default_rng(1).permutation(len(imgs))
    assert not np.array_equal(perm, np.arange(len(imgs)))
    shuffled = roma_amd.preprocess_images([imgs[j] for j in perm], BATCH_TARGETS, device="cuda:0")
    again = roma_amd.preprocess_images(imgs, BATCH_TARGETS, device="cuda:0")
    for t in range(2):
        assert same_bits(shuffled[t], outs[t][torch.as_tensor(perm, device=outs[t].device)].cpu())
        assert same_bits(again[t], outs[t].cpu())
    # one target out of a pair = the single-size call
    one = roma_amd.preprocess_images(imgs, BATCH_TARGETS[1], device="cuda:0")
    assert same_bits(one, outs[1].cpu())


def test_device_tensors_paths_and_pil_images_give_the_same_bits_as_host_arrays(built_lib):
    from PIL import Image
    import roma_amd
    imgs = [img for _, img, _ in pc.cases()]
    ref = batch_reference()
    dev = torch.device("cuda:0")
    on_device = [torch.as_tensor(np.array(img), device=dev) for img in imgs]
    outs = roma_amd.preprocess_images(on_device, BATCH_TARGETS)
    assert outs[0].device == dev
    # host arrays, host tensors, device tensors, PIL images and a path in one call
    mixed = [on_device[i] if i % 3 == 0 else (torch.as_tensor(np.array(imgs[i])) if i % 3 == 1 else Image.fromarray(imgs[i])) for i in range(len(imgs))]
    mixed[0] = os.path.join(GOLDEN, "pair_A.png")
    outs_mixed = roma_amd.preprocess_images(mixed, BATCH_TARGETS, device=dev)
    for t in range(2):
        for i in range(len(imgs)):
            assert same_bits(outs[t][i], ref[t][i]), (BATCH_TARGETS[t], CASE_IDS[i])
            assert same_bits(outs_mixed[t][i], ref[t][i]), (BATCH_TARGETS[t], CASE_IDS[i])


def _crops():
    """three different crops per side of the golden pair, of three different sizes"""
    from PIL import Image
    a = np.array(Image.open(os.path.join(GOLDEN, "pair_A.png")).convert("RGB"))
    b = np.array(Image.open(os.path.join(GOLDEN, "pair_B.png")).convert("RGB"))
    boxes = ((0, 0, 480, 640), (33, 57, 301, 403), (120, 200, 199, 251))  # y0, x0, h, w
    cut = lambda im: [np.ascontiguousarray(im[y:y + h, x:x + w]) for y, x, h, w in boxes]  # noqa: E731
    return cut(a), cut(b)


def _stack(imgs, hw):
    from PIL import Image
    from roma_amd.matcher import _pil_to_normalised
    return torch.stack([_pil_to_normalised(Image.fromarray(im), hw) for im in imgs])


def test_match_images_equals_match_on_the_golden_pair(built_lib, weights0):
    from roma_amd import roma_model
    sd, dsd = weights0
    pa, pb = os.path.join(GOLDEN, "pair_A.png"), os.path.join(GOLDEN, "pair_B.png")
    m = roma_model((112, 112), True, device="cuda:0", weights=sd, dinov2_weights=dsd, amp_dtype=torch.float32, symmetric=True,
                   upsample_res=(168, 168))
    warp, cert = m.match(pa, pb)
    warp2, cert2 = m.match_images(pa, pb)
    assert tuple(warp2.shape) == (1, 168, 336, 4) and tuple(cert2.shape) == (1, 168, 336)
    assert torch.equal(warp2, warp) and torch.equal(cert2, cert)
    m.upsample_preds = False  # coarse only: one target
    warp, cert = m.match(pa, pb)
    warp2, cert2 = m.match_images(pa, pb)
    assert tuple(warp2.shape) == (1, 112, 224, 4) and torch.equal(warp2, warp) and torch.equal(cert2, cert)


@pytest.mark.parametrize("amp", [torch.float32, torch.float16], ids=["f32", "default_16bit"])
def test_match_images_batch_of_three_chunked_by_max_batch(built_lib, weights0, amp):
    """the same model call on inputs that must be identical: match() on the tensor batch stacked from the host path"""
    from roma_amd import roma_model
    sd, dsd = weights0
    crops_a, crops_b = _crops()
    m = roma_model((112, 112), True, device="cuda:0", weights=sd, dinov2_weights=dsd, amp_dtype=amp, symmetric=True,
                   upsample_res=(168, 168), max_batch=2)
    dev = m.device
    warp, cert = m.match(_stack(crops_a, (112, 112)).to(dev), _stack(crops_b, (112, 112)).to(dev),
                         im_A_high_res=_stack(crops_a, (168, 168)).to(dev), im_B_high_res=_stack(crops_b, (168, 168)).to(dev))
    warp2, cert2 = m.match_images(crops_a, crops_b)
    assert tuple(warp2.shape) == (3, 168, 336, 4)
    assert torch.equal(warp2, warp) and torch.equal(cert2, cert)
