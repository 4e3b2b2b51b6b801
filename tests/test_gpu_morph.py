"""roma_amd.render_morph (csrc/morph.hip) on the device against tools/morph_ref.py, the numpy float32 oracle that
tests/test_cpu_morph.py holds to the reference's recorded frames, and against those frames themselves, on the scene of
tests/morph_cases.py.  Both sides run the same correctly rounded float32 operations in the same order: the expected difference of
the float frames is 0, the bound 2e-6; uint8 frames are compared with the reference's under the rule of morph_cases.check_uint8."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import morph_cases as cases

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()  # a copy: the scene's arrays are read-only


def same_bits(a, b):
    a, b = a.contiguous().cpu().numpy(), b.contiguous().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def scene_dev():
    return {k: dev(v) for k, v in cases.scene().items()}


@pytest.fixture(scope="module")
def frames(scene_dev):
    """the plain call in both output forms, shared and left unchanged: (uint8 [B, T, H, W, 3], float32 [B, T, 3, H, W])"""
    import roma_amd
    s = scene_dev
    u8 = roma_amd.render_morph(s["warp"], s["image"], s["ts"])
    fl = roma_amd.render_morph(s["warp"], s["image"], s["ts"], dtype=torch.float32)
    T = len(cases.scene()["ts"])
    assert u8.shape == (cases.B, T, cases.H, cases.W, 3) and u8.dtype == torch.uint8 and u8.is_cuda
    assert fl.shape == (cases.B, T, 3, cases.H, cases.W) and fl.dtype == torch.float32
    return u8, fl


def float_difference(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and not np.isnan(got).any()
    worst = float(np.abs(got - want).max())
    print(f"{what}: worst float difference {worst:.3e}, {int((got != want).sum())} of {got.size} values differ")
    return worst


# ------------------------------------------------------------------------------------ against the oracle and the reference
def test_float_frames_equal_the_oracle(frames):
    want, want_u8 = cases.oracle("plain")
    worst = float_difference(frames[1], want, "device vs oracle (plain)")
    assert worst <= cases.FLOAT_ATOL
    # the uint8 form is the float form through the truncation: equal floats, equal bytes
    d = np.abs(frames[0].cpu().numpy().astype(np.int16) - want_u8.astype(np.int16))
    assert d.max() <= 1 and (worst > 0 or d.max() == 0)


def test_frames_that_all_start_dword_aligned(scene_dev):
    """36 x 52 = 1872 pixels, a multiple of 4: every frame starts dword aligned, so every full wave of the uint8 form stores dwords
    (on the 37 x 53 scene one frame in four does); the crop is a strided view, read in place"""
    import roma_amd
    import morph_ref as mr
    s, sc = scene_dev, cases.scene()
    ts = sc["ts"][[1, 2, 8]]
    fl = roma_amd.render_morph(s["warp"][:, :36, :52], s["image"], ts, certainty=s["certainty"][:, :36, :52], dtype=torch.float32)
    u8 = roma_amd.render_morph(s["warp"][:, :36, :52], s["image"], ts, certainty=s["certainty"][:, :36, :52])
    want = [mr.render_morph(sc["warp"][b, :36, :52], sc["image"][b], ts, sc["certainty"][b, :36, :52], 1.0) for b in range(cases.B)]
    worst = float_difference(fl, np.stack([w[0] for w in want]), "device vs oracle (36 x 52)")
    assert worst <= cases.FLOAT_ATOL
    d = np.abs(u8.cpu().numpy().astype(np.int16) - np.stack([w[1] for w in want]).astype(np.int16))
    assert d.max() <= 1 and (worst > 0 or d.max() == 0)


def test_float_frames_are_within_the_bound_of_the_reference(frames):
    assert float_difference(frames[1], cases.golden()["ref_float"], "device vs reference (plain)") <= cases.FLOAT_ATOL


def test_uint8_frames_match_the_reference(frames):
    g = cases.golden()
    cases.check_uint8(frames[0].cpu().numpy(), g["ref_u8"], g["ref_float"], "device vs reference (plain)")


def test_certainty_blend_matches_the_oracle_and_the_reference(scene_dev):
    import roma_amd
    s, g = scene_dev, cases.golden()
    kw = dict(certainty=s["certainty"], background=cases.BACKGROUND)
    fl = roma_amd.render_morph(s["warp"], s["image"], s["ts_cert"], dtype=torch.float32, **kw)
    u8 = roma_amd.render_morph(s["warp"], s["image"], s["ts_cert"], **kw)
    assert float_difference(fl, cases.oracle("cert")[0], "device vs oracle (certainty)") <= cases.FLOAT_ATOL
    assert float_difference(fl, g["ref_cert_float"], "device vs reference (certainty)") <= cases.FLOAT_ATOL
    cases.check_uint8(u8.cpu().numpy(), g["ref_cert_u8"], g["ref_cert_float"], "device vs reference (certainty)")
    # another background than white, against the oracle alone
    import morph_ref as mr
    sc = cases.scene()
    got = roma_amd.render_morph(s["warp"][1], s["image"][1], s["ts_cert"], certainty=s["certainty"][1], background=0.25, dtype=torch.float32)
    want = mr.render_morph(sc["warp"][1], sc["image"][1], sc["ts_cert"], sc["certainty"][1], 0.25)[0]
    assert float_difference(got, want, "device vs oracle (background 0.25)") <= cases.FLOAT_ATOL


def test_one_frame_and_one_frame_more_than_a_chunk(scene_dev):
    import roma_amd
    from roma_amd import render
    s = scene_dev
    for name, ts in zip(("one", "chunk"), cases.extra_times(render.FRAME_CHUNK)):
        assert len(ts) == (1 if name == "one" else render.FRAME_CHUNK + 1)
        want_fl, want_u8 = cases.oracle(name, render.FRAME_CHUNK)
        fl = roma_amd.render_morph(s["warp"], s["image"], ts, dtype=torch.float32)
        u8 = roma_amd.render_morph(s["warp"], s["image"], ts)
        worst = float_difference(fl, want_fl, f"device vs oracle (T = {len(ts)})")
        assert worst <= cases.FLOAT_ATOL
        d = np.abs(u8.cpu().numpy().astype(np.int16) - want_u8.astype(np.int16))
        assert d.max() <= 1 and (worst > 0 or d.max() == 0)


# ------------------------------------------------------------------------------------------------ API forms and determinism
def test_uint8_picture_gives_the_bits_of_the_float_picture(scene_dev):
    import roma_amd
    import morph_ref as mr
    s, sc = scene_dev, cases.scene()
    as_float = dev(np.stack([mr.image_f32(im) for im in sc["image_u8"]]))
    for dtype in (torch.uint8, torch.float32):
        a = roma_amd.render_morph(s["warp"], s["image_u8"], s["ts"], dtype=dtype)
        b = roma_amd.render_morph(s["warp"], as_float, s["ts"], dtype=dtype)
        assert same_bits(a, b)
    assert float_difference(b, cases.oracle("u8")[0], "device vs oracle (uint8 picture)") <= cases.FLOAT_ATOL


def test_strided_left_half_of_a_symmetric_warp_is_read_in_place(scene_dev, frames):
    import roma_amd
    s = scene_dev
    sym = torch.cat([s["warp"], torch.randn_like(s["warp"])], dim=2)  # [B, H, 2W, 4]
    left = sym[:, :, :cases.W]
    assert not left.is_contiguous() and left.stride(-1) == 1 and left.stride(-2) == 4
    wide = torch.cat([s["certainty"], torch.rand_like(s["certainty"])], dim=2)[:, :, :cases.W]
    assert not wide.is_contiguous()
    assert same_bits(roma_amd.render_morph(left, s["image"], s["ts"]), frames[0])
    assert same_bits(roma_amd.render_morph(left, s["image"], s["ts"], dtype=torch.float32), frames[1])
    a = roma_amd.render_morph(left, s["image"], s["ts_cert"], certainty=wide)
    b = roma_amd.render_morph(s["warp"], s["image"], s["ts_cert"], certainty=s["certainty"])
    assert same_bits(a, b)


def test_batch_single_calls_and_runs_are_bit_identical(scene_dev, frames):
    import roma_amd
    s = scene_dev
    assert same_bits(roma_amd.render_morph(s["warp"], s["image"], s["ts"]), frames[0])  # run to run
    for b in range(cases.B):
        one = roma_amd.render_morph(s["warp"][b], s["image"][b], s["ts"])  # no batch axis in, none out
        assert one.shape == frames[0].shape[1:] and same_bits(one, frames[0][b])
        one = roma_amd.render_morph(s["warp"][b:b + 1], s["image"][b:b + 1], s["ts"], dtype=torch.float32)
        assert one.shape[0] == 1 and same_bits(one[0], frames[1][b])


def test_host_and_device_times_give_the_same_bits(scene_dev, frames):
    import roma_amd
    s, ts = scene_dev, cases.scene()["ts"]
    for form in (list(ts), np.array(ts), torch.from_numpy(np.array(ts)), s["ts"]):
        assert same_bits(roma_amd.render_morph(s["warp"], s["image"], form), frames[0])


def test_matcher_methods_forward(scene_dev, frames):
    from roma_amd.matcher import RegressionMatcher
    from roma_amd.tiny import TinyRoMa
    s = scene_dev
    for cls in (RegressionMatcher, TinyRoMa):
        assert same_bits(cls.__new__(cls).render_morph(s["warp"], s["image"], s["ts"], dtype=torch.float32), frames[1])


def test_host_tensors_raise(scene_dev):
    import roma_amd
    from roma_amd import _lib
    s, sc = scene_dev, cases.scene()
    host = {k: torch.from_numpy(np.array(v)) for k, v in sc.items()}
    for kw in (dict(warp=host["warp"]), dict(image=host["image"]), dict(certainty=host["certainty"])):
        a = {"warp": s["warp"], "image": s["image"], **kw}
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            roma_amd.render_morph(a.pop("warp"), a.pop("image"), sc["ts"], **a)


@pytest.mark.parametrize("out_f32", [0, 1])
def test_nothing_is_written_outside_the_frames(scene_dev, frames, out_f32):
    """the C entry point on an output over-allocated by one frame row of guard values on each side: 0xAB bytes (uint8) or NaN"""
    from roma_amd import _lib
    from roma_amd._lib import _ptr, _stream
    s = scene_dev
    T = int(s["ts"].shape[0])
    n_out = cases.B * T * cases.H * cases.W * 3
    row = cases.W * 3
    if out_f32:
        buf = torch.full((n_out + 2 * row,), float("nan"), device="cuda", dtype=torch.float32)
    else:
        buf = torch.full((n_out + 2 * row,), 0xAB, device="cuda", dtype=torch.uint8)
    out = buf[row:row + n_out]
    lib = _lib.load()
    ws_bytes = int(lib.roma_op_render_morph_workspace(cases.B, cases.IM_H, cases.IM_W, T))
    ws = torch.empty(ws_bytes // 8 + 2, device="cuda", dtype=torch.float64)
    _lib.check(lib.roma_op_render_morph(_ptr(s["warp"]), cases.H * cases.W * 4, cases.W * 4, _ptr(s["image"]), 0, _ptr(s["ts"]), None, 0, 0,
                                        1.0, cases.B, T, cases.H, cases.W, cases.IM_H, cases.IM_W, _ptr(out), out_f32, _ptr(ws), ws_bytes,
                                        _stream(buf.device)))
    torch.cuda.synchronize()
    assert same_bits(out.reshape(frames[out_f32].shape), frames[out_f32])
    guards = torch.cat([buf[:row], buf[row + n_out:]])
    assert bool(torch.isnan(guards).all()) if out_f32 else bool((guards == 0xAB).all())
