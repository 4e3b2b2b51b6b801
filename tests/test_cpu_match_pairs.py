"""Host side of the cached per-image features (roma_amd/encoded.py): the pair list, the pack layout and the pair validation.
No GPU: pack_layout is a pure Python restatement of csrc/encoded.hip::pack_layout."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_all_pairs_order_and_count():
    from roma_amd.encoded import all_pairs
    assert all_pairs(0) == [] and all_pairs(1) == []
    assert all_pairs(2) == [(0, 1)]
    assert all_pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for n in (3, 8, 13):
        p = all_pairs(n)
        assert len(p) == n * (n - 1) // 2 and p == sorted(p) and all(i < j for i, j in p) and len(set(p)) == len(p)
    with pytest.raises(ValueError):
        all_pairs(-1)


@pytest.mark.parametrize("coarse,up,itemsize", [((112, 112), (168, 168), 2), ((112, 112), (168, 168), 4), ((560, 560), (864, 864), 2),
                                                ((126, 154), (182, 198), 4), ((112, 140), None, 2), ((560, 560), (0, 0), 4)])
def test_pack_layout_segments_are_aligned_monotone_and_disjoint(coarse, up, itemsize):
    from roma_amd.encoded import pack_layout
    L = pack_layout(coarse, up, itemsize)
    segs = L["segments"]
    has_up = up is not None and up[0] > 0
    assert [(s["pass"], s["scale"]) for s in segs] == [(0, 16), (0, 8), (0, 4), (0, 2), (0, 1)] + ([(1, 8), (1, 4), (1, 2), (1, 1)] if has_up else [])
    end = 0
    for s in segs:
        assert s["offset"] % 256 == 0 and s["offset"] >= end  # aligned, monotone, no overlap with the one before
        assert s["bytes"] == s["hw"] * s["ldf"] * itemsize and s["bytes"] % 16 == 0 and s["ldf"] % 8 == 0
        end = s["offset"] + s["bytes"]
    assert L["total"] % 256 == 0 and end <= L["total"] < end + 256
    assert L["coarse_bytes"] == (segs[5]["offset"] if has_up else L["total"])


def _arch_proj_cout():
    src = open(os.path.join(ROOT, "roma_amd", "csrc", "arch.h")).read()
    m = re.search(r"PROJ_COUT\[5\]\s*=\s*\{([^}]*)\}", src)
    return [int(v) for v in m.group(1).split(",")]


def test_pack_layout_totals_from_arch_h():
    """The sums written out: channels from arch.h's PROJ_COUT (512, 512, 256, 64, 9 -> row strides 512, 512, 256, 64, 16)."""
    from roma_amd import encoded
    assert _arch_proj_cout() == [512, 512, 256, 64, 9] == list(encoded.PROJ_COUT)

    def r256(v):
        return (v + 255) // 256 * 256
    # 112 -> 168, f32: token grid 8 x 8; coarse maps 14^2, 28^2, 56^2, 112^2; upsample maps 21^2, 42^2, 84^2, 168^2
    tot = 0
    for hw, ld in ((64, 512), (14 * 14, 512), (28 * 28, 256), (56 * 56, 64), (112 * 112, 16),
                   (21 * 21, 512), (42 * 42, 256), (84 * 84, 64), (168 * 168, 16)):
        tot = r256(tot + hw * ld * 4)
    assert encoded.pack_layout((112, 112), (168, 168), 4)["total"] == tot == 9263104
    # 560 -> 864, 16 bit: token grid 40 x 40; 70^2, 140^2, 280^2, 560^2; 108^2, 216^2, 432^2, 864^2
    tot = 0
    for hw, ld in ((1600, 512), (70 * 70, 512), (140 * 140, 256), (280 * 280, 64), (560 * 560, 16),
                   (108 * 108, 512), (216 * 216, 256), (432 * 432, 64), (864 * 864, 16)):
        tot = r256(tot + hw * ld * 2)
    L = encoded.pack_layout((560, 560), (864, 864), 2)
    assert L["total"] == tot == 120369152  # "about 120 MB per image"
    assert encoded.pack_layout((560, 560), (864, 864), 4)["total"] == 2 * tot  # every segment doubles, 256 divides both
    assert encoded.pack_layout((560, 560), None, 2)["total"] == L["coarse_bytes"]
    with pytest.raises(ValueError):
        encoded.pack_layout((560, 560), None, 3)


def test_pair_validation():
    import torch
    from roma_amd.encoded import all_pairs, check_pairs
    a = check_pairs([(2, 0), (1, 3)], 4)
    assert a.dtype == np.int32 and a.shape == (2, 2) and a.flags["C_CONTIGUOUS"] and a.tolist() == [[2, 0], [1, 3]]
    assert check_pairs(None, 4).tolist() == [list(p) for p in all_pairs(4)]
    assert check_pairs(np.array([[0, 0]], dtype=np.uint8), 1).tolist() == [[0, 0]]  # an image against itself is a valid pair
    assert check_pairs(torch.tensor([[1, 0]]), 2).tolist() == [[1, 0]]
    for bad in ([(0, -1)], [(4, 0)], np.array([[0, 1], [1, 4]])):                    # out of range: -1 and N
        with pytest.raises(ValueError, match="outside"):
            check_pairs(bad, 4)
    for bad in ([0, 1, 2], [[0, 1, 2]], np.zeros((2, 2, 2), dtype=np.int64)):         # shape
        with pytest.raises(ValueError, match="shape"):
            check_pairs(bad, 4)
    for bad in ([(0.0, 1.0)], np.array([[0, 1]], dtype=np.float32), [(True, False)]):  # dtype
        with pytest.raises(ValueError, match="integers"):
            check_pairs(bad, 4)
    for bad in ([], np.zeros((0, 2), dtype=np.int64)):                                 # empty
        with pytest.raises(ValueError, match="empty"):
            check_pairs(bad, 4)
    with pytest.raises(ValueError, match="empty"):
        check_pairs(None, 1)  # one image has no pair


def test_public_surface():
    import roma_amd
    from roma_amd import RegressionMatcher
    for name in ("EncodedImages", "all_pairs", "pack_layout"):
        assert name in roma_amd.__all__ and hasattr(roma_amd, name)
    for name in ("encode_images", "match_pairs", "match_image_set", "encoded_bytes"):
        assert callable(getattr(RegressionMatcher, name))
    from roma_amd import _lib
    for name in ("roma_encoded_bytes", "roma_encode", "roma_match_encoded"):
        assert name in _lib.SIGNATURES
