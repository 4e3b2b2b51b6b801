"""tools/pil_resample_ref.py (the numpy restatement of Pillow's 8-bit bicubic resize that csrc/preprocess.hip implements) against
Pillow itself and against the matcher's host path, bit for bit, on the cases tests/test_gpu_preprocess.py runs; the C ABI of
roma_op_preprocess (dlopen only); the Python argument errors; the kernels' register metadata.  No GPU."""
import ctypes as C
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import pil_resample_ref as ref  # noqa: E402
import preprocess_cases as pc  # noqa: E402

NEW_SYMBOLS = ("roma_op_preprocess", "roma_op_preprocess_workspace")
CASE_IDS = [c[0] for c in pc.cases()]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_the_case_list_is_the_one_the_issue_sets():
    got = [(tuple(img.shape[:2]), hw) for _, img, hw in pc.cases()]
    assert got == [((480, 640), (56, 70)), ((37, 53), (70, 84)), ((480, 640), (480, 98)), ((480, 640), (42, 640)),
                   ((480, 640), (560, 560)), ((28, 42), (28, 42)), ((5, 3), (28, 42)), ((301, 1), (14, 14)), ((97, 1031), (28, 42)),
                   ((64, 80), (42, 56)), ((20, 24), (56, 70)), ((16, 16), (16, 16))]
    by = {name: img for name, img, _ in pc.cases()}
    for name in pc.CLAMP_CASES:
        assert set(np.unique(by[name])) == {0, 255}
    for c in range(3):
        assert sorted(by["every_byte"][:, :, c].reshape(-1)) == list(range(256))
    _, n, _ = ref.coefficients(1031, 42)
    assert n.max() == 99


@pytest.mark.parametrize("case", pc.cases(), ids=CASE_IDS)
def test_oracle_equals_pillow_bit_for_bit(case):
    from PIL import Image
    _, img, (h, w) = case
    want = np.array(Image.fromarray(img).resize((w, h), resample=Image.BICUBIC))
    got = ref.resize(img, (h, w))
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("case", pc.cases(), ids=CASE_IDS)
def test_oracle_normalised_output_equals_the_host_path_bit_for_bit(case):
    from PIL import Image
    from roma_amd.matcher import _pil_to_normalised
    _, img, hw = case
    want = _pil_to_normalised(Image.fromarray(img), hw).numpy()
    assert np.array_equal(bits(ref.preprocess(img, hw, normalize=True)), bits(want))
    assert np.array_equal(bits(pc.reference(img, hw, True)), bits(want))
    # normalize=False: the / 255 of visualize_warp (uint8 tensor / 255 in float32)
    plain = (torch.tensor(ref.resize(img, hw)) / 255).permute(2, 0, 1).numpy()
    assert np.array_equal(bits(ref.preprocess(img, hw, normalize=False)), bits(plain))
    assert np.array_equal(bits(pc.reference(img, hw, False)), bits(plain))


def test_normalisation_table_covers_every_byte_in_every_channel():
    from roma_amd.matcher import IMAGENET_MEAN, IMAGENET_STD
    t = ref.normalisation_table(True)
    u = np.arange(256, dtype=np.float32)[None, :, None].repeat(3, 0)  # [3, 256, 1] as a CHW image
    want = (u / np.float32(255.0) - np.array(IMAGENET_MEAN, dtype=np.float32)[:, None, None]) / np.array(IMAGENET_STD, dtype=np.float32)[:, None, None]
    assert t.shape == (3, 256) and np.array_equal(bits(t), bits(want[:, :, 0]))
    assert np.array_equal(bits(ref.normalisation_table(False)), bits((u / np.float32(255.0))[:, :, 0]))
    _, img, hw = [c for c in pc.cases() if c[0] == "every_byte"][0]
    for normalize in (True, False):  # the every_byte case reaches all 768 entries
        out, tab = ref.preprocess(img, hw, normalize), ref.normalisation_table(normalize)
        for c in range(3):
            assert set(bits(out[c]).reshape(-1)) == set(bits(tab[c]))


@pytest.mark.parametrize("name", pc.CLAMP_CASES)
def test_clamp_cases_saturate_at_both_ends(name):
    """both clamps must fire: at least one 0 and one 255 in the result whose unclamped sum lay outside [0, 255]"""
    _, img, hw = [c for c in pc.cases() if c[0] == name][0]
    saturated = [0, 0]
    out = ref.resize(img, hw, saturated)
    assert saturated[0] >= 1 and saturated[1] >= 1, saturated
    # in the LAST pass too, so that the bytes of the result themselves are clamped ones
    mid = ref.resize(img, (img.shape[0], hw[1]))
    last = [0, 0]
    assert np.array_equal(ref.resize(mid, hw, last), out)
    assert last[0] >= 1 and last[1] >= 1 and (out == 0).sum() >= last[0] and (out == 255).sum() >= last[1], last


def test_pass_order_and_intermediate_rounding_matter():
    """vertical-first, or one exact pass, gives other bytes: the order and the uint8 intermediate are part of the definition"""
    _, img, (h, w) = pc.cases()[0]
    want = ref.resize(img, (h, w))
    other = ref.resize(ref.resize(img, (h, img.shape[1])), (h, w))
    assert not np.array_equal(want, other)


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert len(_lib.SIGNATURES["roma_op_preprocess_workspace"][1]) == 4
    assert len(_lib.SIGNATURES["roma_op_preprocess"][1]) == 12
    assert "horizontal first" in header.lower() and "PRECISION_BITS = 22" in header


def _desc(*rows):
    a = np.array(rows, dtype=np.int64).reshape(-1, 3)
    return a, a.ctypes.data_as(C.c_void_p)


def _targets(*hw):
    return (C.c_int * len(hw))(*hw)


def test_workspace_size_is_monotone_in_the_inputs(built_lib):
    lib = built_lib

    def ws(sizes, targets):
        keep, d = _desc(*[(0, h, w) for h, w in sizes])
        return lib.roma_op_preprocess_workspace(d, len(sizes), _targets(*targets), len(targets) // 2)
    base = ws([(480, 640)], (56, 70))
    assert base > 768 * 4
    assert ws([(480, 640)] * 2, (56, 70)) > base               # more images
    assert ws([(480, 640), (37, 53)], (56, 70)) == ws([(480, 640)] * 2, (56, 70))  # equal slots, sized by the largest image
    assert ws([(481, 640)], (56, 70)) >= base and ws([(480, 641)], (56, 70)) >= base and ws([(960, 1280)], (56, 70)) > base
    assert ws([(480, 640)], (56, 70, 84, 98)) > base           # a second target
    prev = 0
    for n in range(1, 6):
        cur = ws([(480, 640)] * n, (56, 70, 84, 98))
        assert cur > prev
        prev = cur


def test_descriptors_are_validated_before_device_work(built_lib):
    lib = built_lib
    p = 64  # any non-null aligned address: validation must fail before it is used
    good_rows = [(0, 480, 640), (921600, 37, 53)]
    total = 921600 + 3 * 37 * 53

    def call(*, rows=good_rows, src=p, src_bytes=total, host=True, dev=p, targets=(56, 70, 84, 98), n_targets=2, out0=p, out1=p, ws=p,
             tptr=True):
        keep, d = _desc(*rows)
        t = _targets(*targets)
        return lib.roma_op_preprocess(src, src_bytes, d if host else None, dev, len(rows), t if tptr else None, n_targets, 1, out0, out1,
                                      ws, None)
    bad = [
        (dict(src_bytes=total - 1), b"src_bytes"),                          # offset + 3 H W > src_bytes
        (dict(rows=[(0, 480, 640), (921601, 37, 53)]), b"src_bytes"),
        (dict(rows=[(1 << 62, 480, 640)]), b"src_bytes"),
        (dict(rows=[(-1, 480, 640)]), b"offset"),
        (dict(rows=[(0, 0, 640)]), b"size"), (dict(rows=[(0, 480, 0)]), b"size"), (dict(rows=[(0, -5, 640)]), b"size"),
        (dict(rows=[(0, 32769, 1)], src_bytes=1 << 40), b"size"), (dict(rows=[(0, 1, 32769)], src_bytes=1 << 40), b"size"),
        (dict(targets=(0, 70, 84, 98)), b"target"), (dict(targets=(56, 70, 84, -1)), b"target"), (dict(targets=(56, 0), n_targets=1), b"target"),
        (dict(n_targets=0), b"n_targets"), (dict(n_targets=3), b"n_targets"), (dict(n_targets=-1), b"n_targets"),
        (dict(src=None), b"null"), (dict(host=False), b"null"), (dict(dev=None), b"null"), (dict(tptr=False), b"null"),
        (dict(out0=None), b"null"), (dict(out1=None), b"null"), (dict(ws=None), b"null"),
        (dict(rows=[]), b"n_images"),
        (dict(src=p + 1), b"aligned"), (dict(ws=p + 8), b"aligned"),
    ]
    for kw, word in bad:
        assert call(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    # the workspace query refuses the same descriptors and targets
    keep, d = _desc((0, 0, 640))
    assert lib.roma_op_preprocess_workspace(d, 1, _targets(56, 70), 1) < 0 and b"size" in lib.roma_last_error()
    keep, d = _desc((0, 480, 640))
    assert lib.roma_op_preprocess_workspace(d, 1, _targets(56, 70), 3) < 0 and b"n_targets" in lib.roma_last_error()
    assert lib.roma_op_preprocess_workspace(d, 1, _targets(0, 70), 1) < 0 and b"target" in lib.roma_last_error()
    assert lib.roma_op_preprocess_workspace(None, 1, _targets(56, 70), 1) < 0 and b"null" in lib.roma_last_error()
    # the largest sizes are accepted by the query (the sizes of the plan are 64-bit)
    keep, d = _desc((0, 32768, 32768))
    assert lib.roma_op_preprocess_workspace(d, 1, _targets(32768, 32768, 1, 1), 2) > 0


def test_python_argument_errors_fire_without_a_device():
    from PIL import Image
    import roma_amd
    from roma_amd import _lib
    from roma_amd.matcher import RegressionMatcher
    assert "preprocess_images" in roma_amd.__all__ and callable(roma_amd.preprocess_images)
    assert callable(RegressionMatcher.match_images)
    ok = np.zeros((8, 9, 3), dtype=np.uint8)
    for images, word in (([], "empty"), ([ok.astype(np.float32)], "dtype"), ([torch.zeros(8, 9, 3)], "dtype"),
                         ([ok[:, :, 0]], "rank"), ([torch.zeros(1, 8, 9, 3, dtype=torch.uint8)], "rank"),
                         ([np.zeros((8, 9, 4), dtype=np.uint8)], "channels"), ([torch.zeros(3, 8, 9, dtype=torch.uint8)], "channels"),
                         ([ok, np.zeros((8, 9, 1), dtype=np.uint8)], "image 1"), ([None], "NoneType"), (ok, "sequence")):
        with pytest.raises(ValueError, match=word):
            roma_amd.preprocess_images(images, (14, 14))
    for sizes in ((14,), (14, 14, 14), ((14, 14), (28, 28), (42, 42)), (0, 14), ((14, 14), (14, -1)), 14, (14.0, 14)):
        with pytest.raises(ValueError, match="sizes"):
            roma_amd.preprocess_images([ok], sizes)
    # the exceptions of match() for 16-bit and non-RGB images (matcher._check_input)
    with pytest.raises(NotImplementedError, match="non-RGB"):
        roma_amd.preprocess_images([Image.new("L", (9, 8))], (14, 14))
    with pytest.raises(NotImplementedError, match="non-RGB"):
        roma_amd.preprocess_images([Image.new("RGBA", (9, 8))], (14, 14))
    # valid arguments and a host device: there is no CPU path
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        roma_amd.preprocess_images([ok], (14, 14), device="cpu")
    m = RegressionMatcher.__new__(RegressionMatcher)
    m.h_resized = m.w_resized = 112
    m.upsample_preds, m.upsample_res, m.device = True, (168, 168), torch.device("cpu")
    with pytest.raises(ValueError, match="equal length"):
        m.match_images([ok, ok], [ok])
    with pytest.raises(ValueError, match="equal length"):
        m.match_images([ok], ok)
    with pytest.raises(ValueError, match="empty"):
        m.match_images([], [])
    with pytest.raises(ValueError, match="dtype"):
        m.match_images(ok, ok.astype(np.float32))
    with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
        m.match_images(ok, os.path.join(GOLDEN, "pair_B.png"))


def test_16_bit_image_files_are_refused_like_match_does(tmp_path):
    from PIL import Image
    import roma_amd
    path = str(tmp_path / "deep.png")
    Image.fromarray(np.arange(72, dtype=np.uint16).reshape(8, 9)).save(path)
    assert Image.open(path).mode == "I;16"
    with pytest.raises(NotImplementedError, match="16 bit"):
        roma_amd.preprocess_images([path], (14, 14))


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_preprocess_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "preprocess.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/preprocess.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["preprocess_coeff_kernel", "preprocess_horizontal_kernel", "preprocess_vertical_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
