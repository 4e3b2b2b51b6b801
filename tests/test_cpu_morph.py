"""tools/morph_ref.py (the oracle of roma_amd.render_morph) against the frames that torch's grid_sample and the unmodified reference's
tensor_to_pil made of the scene of tests/morph_cases.py (tests/golden/morph_reference.npz), the conditions tests/test_gpu_morph.py
puts on that scene, and the C ABI and Python surface of roma_op_render_morph (dlopen only).  No GPU."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import morph_cases as cases

sys.path.insert(0, os.path.join(ROOT, "tools"))
import morph_ref as mr  # noqa: E402

NEW_SYMBOLS = ("roma_op_render_morph", "roma_op_render_morph_workspace", "roma_op_render_morph_frame_chunk")


# ------------------------------------------------------------------------------------------------- oracle against the golden
def test_recorded_scene_is_the_generated_one():
    """the golden holds the bits the reference ran on; the generator reproduces them up to this machine's libm"""
    built, s = cases.build_scene(), cases.scene()
    for k in cases.INPUTS:
        assert built[k].shape == s[k].shape and built[k].dtype == s[k].dtype, k
        assert np.allclose(built[k], s[k], rtol=0, atol=1e-6), k
    assert s["warp"].shape == (cases.B, 37, 53, 4) and s["image"].shape == (cases.B, 3, 29, 41) and s["image_u8"].shape == (cases.B, 29, 41, 3)
    assert s["ts"].dtype == np.float64 and len(s["ts"]) == 9 and s["ts"][0] == 1.0 and s["ts"][3] == 0.0
    assert list(s["ts"][7:]) == [1.5, -0.25] and np.array_equal(s["ts_cert"], s["ts"][[1, 4, 7]])


@pytest.mark.parametrize("name, ref", [("plain", ""), ("cert", "cert_")])
def test_oracle_matches_the_reference_frames(name, ref):
    g = cases.golden()
    fl, u8 = cases.oracle(name)
    ref_fl, ref_u8 = g[f"ref_{ref}float"], g[f"ref_{ref}u8"]
    assert fl.shape == ref_fl.shape and fl.dtype == np.float32 and not np.isnan(fl).any()
    worst = float(np.abs(fl - ref_fl).max())
    print(f"oracle vs reference ({name}): worst float difference {worst:.3e}, {float((fl != ref_fl).mean()) * 100:.1f} % of the values differ")
    assert worst <= cases.FLOAT_ATOL
    cases.check_uint8(u8, ref_u8, ref_fl, f"oracle vs reference ({name})")


def test_scene_takes_every_branch():
    s = cases.scene()
    n = cases.H * cases.W
    assert cases.W % 2 == 1 and n % 256 not in (0, 255) and n > 256 * 4 and (n * 3) % 4 != 0  # a partial wave, two workgroups, every dword phase
    w0, w1 = mr.frame_weights(s["ts"])
    assert (w0.astype(np.float64) != 1.0 - s["ts"]).any() and w0[0] == 0 and w0[3] == 1  # rounding in 1 - t; the end points
    seen = {"all outside": 0, "some outside": 0, "inside": 0}
    for b in range(cases.B):
        for k in range(len(w0)):
            gx = w0[k] * s["warp"][b, ..., 0] + w1[k] * s["warp"][b, ..., 2]
            gy = w0[k] * s["warp"][b, ..., 1] + w1[k] * s["warp"][b, ..., 3]
            ix, iy = ((gx + 1) * cases.IM_W - 1) * 0.5, ((gy + 1) * cases.IM_H - 1) * 0.5
            x0, y0 = np.floor(ix), np.floor(iy)
            n_in = sum(((x0 + dx >= 0) & (x0 + dx < cases.IM_W) & (y0 + dy >= 0) & (y0 + dy < cases.IM_H)).astype(int)
                       for dx in (0, 1) for dy in (0, 1))
            seen["all outside"] += int((n_in == 0).sum())
            seen["some outside"] += int(((n_in > 0) & (n_in < 4)).sum())
            seen["inside"] += int((n_in == 4).sum())
    print("pixel-frames per population:", seen)
    assert all(v > 100 for v in seen.values())
    ce = s["certainty"]
    assert ce.min() == 0.0 and ce.max() == 1.0 and ((ce > 0) & (ce < 1)).mean() > 0.5
    fl, _ = cases.oracle("plain")
    assert 0.05 < float((fl == 0).mean()) < 0.3


def test_uint8_picture_is_the_float_picture_divided_by_255():
    s = cases.scene()
    img = mr.image_f32(s["image_u8"][0])
    assert img.dtype == np.float32 and img.shape == (3, cases.IM_H, cases.IM_W)
    exact = s["image_u8"][0].astype(np.float64).transpose(2, 0, 1) / 255.0
    assert np.array_equal(img, exact.astype(np.float32))  # correctly rounded
    a = mr.render_morph(s["warp"][0], s["image_u8"][0], s["ts"][:2])
    b = mr.render_morph(s["warp"][0], img, s["ts"][:2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_non_finite_coordinates_and_values():
    img = np.full((3, 2, 2), 0.5, dtype=np.float32)
    warp = np.zeros((1, 4, 4), dtype=np.float32)
    warp[0, :, 2] = [np.nan, np.inf, -np.inf, 0.0]
    fl, u8 = mr.render_morph(warp, img, [1.0])
    assert np.array_equal(fl[0, :, 0, :3], np.zeros((3, 3), dtype=np.float32)) and np.all(fl[0, :, 0, 3] == 0.5)
    assert np.array_equal(mr.to_uint8(np.array([np.nan, -1.0, 0.0, 0.999999, 1.0, 7.0, 0.5], dtype=np.float32)), [0, 0, 0, 254, 255, 255, 127])


def test_morph_times_is_the_demo_schedule():
    import roma_amd
    t = roma_amd.morph_times(200)
    assert t.dtype == np.float64 and np.array_equal(t, (1 + np.cos(np.linspace(0, 2 * np.pi, 200))) / 2)
    assert np.array_equal(roma_amd.morph_times(), t) and np.array_equal(roma_amd.morph_times(7), mr.morph_times(7))
    with pytest.raises(ValueError):
        roma_amd.morph_times(0)


# ------------------------------------------------------------------------------------------------------------ C ABI, Python
def test_new_symbols_are_declared_and_exported_by_both_builds(built_lib):
    from roma_amd import _lib, render
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
    assert len(_lib.SIGNATURES["roma_op_render_morph"][1]) == 21
    assert len(_lib.SIGNATURES["roma_op_render_morph_workspace"][1]) == 4
    for fmt in ("bf16", "f16"):
        assert _lib.load(fmt).roma_op_render_morph_frame_chunk() == render.FRAME_CHUNK
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "morph.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "morph" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()  # no packed f32 here


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_c_abi_validates_before_device_work(built_lib, fmt):
    from roma_amd import _lib
    lib = _lib.load(fmt)
    H, W, h, w, T, B = 37, 53, 29, 41, 9, 2
    # addresses that are never used: validation must fail first.  Disjoint ranges, aligned as their types ask.
    WARP, IMG, TS, CERT, OUT, WS = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 8 << 20, 16 << 20

    def call(*, warp=WARP, sb=H * W * 4, sr=W * 4, img=IMG, u8=0, ts=TS, cert=None, cb=H * W, cr=W, bg=1.0, B=B, T=T, H=H, W=W, h=h, w=w,
             out=OUT, f32=0, ws=WS, ws_bytes=1 << 22):
        return lib.roma_op_render_morph(warp, sb, sr, img, u8, ts, cert, cb, cr, bg, B, T, H, W, h, w, out, f32, ws, ws_bytes, None)
    need = lib.roma_op_render_morph_workspace(B, h, w, T)
    assert need == B * (h * w + 1) * 16 + T * 8
    for kw, word in ((dict(warp=None), b"null"), (dict(img=None), b"null"), (dict(ts=None), b"null"), (dict(out=None), b"null"),
                     (dict(ws=None), b"null"), (dict(B=0), b"B"), (dict(B=65536), b"B"), (dict(T=0), b"T"), (dict(T=-4), b"T"),
                     (dict(T=65535 * 32 + 1), b"T"), (dict(H=0), b"warp grid"), (dict(W=32769, sr=4 * 32769), b"warp grid"),
                     (dict(h=0), b"image size"), (dict(w=40000), b"image size"), (dict(u8=2), b"image_u8"), (dict(f32=-1), b"out_f32"),
                     (dict(sr=W * 4 - 4), b"warp strides"), (dict(sr=W * 4 + 2), b"warp strides"), (dict(sb=(H - 1) * W * 4), b"warp strides"),
                     (dict(sb=H * W * 4 + 1), b"warp strides"), (dict(cert=CERT, cr=W - 1), b"certainty strides"),
                     (dict(cert=CERT, cb=H * W - 1), b"certainty strides"), (dict(warp=WARP + 8), b"16-byte"), (dict(ws=WS + 4), b"16-byte"),
                     (dict(ts=TS + 4), b"aligned"), (dict(cert=CERT + 2), b"aligned"), (dict(img=IMG + 1), b"aligned"),
                     (dict(out=OUT + 2, f32=1), b"aligned"), (dict(bg=float("nan")), b"NaN"), (dict(ws_bytes=need - 1), b"workspace"),
                     (dict(out=WARP), b"aliases"), (dict(out=WARP + 4 * (B * H * W * 4) - 1), b"aliases"), (dict(out=IMG - 1), b"aliases"),
                     (dict(out=TS), b"aliases"), (dict(cert=CERT, out=CERT + 64), b"aliases"), (dict(ws=IMG), b"aliases"),
                     (dict(ws=WARP + 16), b"aliases"), (dict(out=WS + 16), b"aliases workspace"),
                     (dict(B=4096, T=65535 * 32, H=32768, W=32768, sb=4 << 30, sr=4 << 15, ws_bytes=1 << 40), b"beyond")):
        assert call(**kw) != 0 and word in lib.roma_last_error(), (kw, lib.roma_last_error())
    # the uint8 picture and the uint8 frames need no alignment: these pass every check but the last, the workspace size
    assert call(img=IMG + 1, u8=1, out=OUT + 3, ws_bytes=8) != 0 and b"workspace" in lib.roma_last_error()
    assert lib.roma_op_render_morph_workspace(1, 864, 1152, 200) == (864 * 1152 + 1) * 16 + 1600
    for bad in ((0, h, w, T), (65536, h, w, T), (B, 0, w, T), (B, h, 32769, T), (B, h, w, 0), (B, h, w, 65535 * 32 + 1)):
        assert lib.roma_op_render_morph_workspace(*bad) == -1


def _host_args():
    return dict(warp=torch.zeros(2, 5, 6, 4), image=torch.zeros(2, 3, 4, 7), ts=[0.0, 0.5])


def test_python_front_end_checks_arguments_and_refuses_host_tensors():
    import roma_amd
    from roma_amd import _lib
    from roma_amd.matcher import RegressionMatcher
    from roma_amd.tiny import TinyRoMa
    for name in ("render_morph", "morph_times"):
        assert name in roma_amd.__all__ and callable(getattr(roma_amd, name))
    assert callable(RegressionMatcher.render_morph) and callable(TinyRoMa.render_morph)
    a = _host_args()
    # shapes and dtypes, before the device is looked at (these are host tensors)
    for bad in (dict(warp=torch.zeros(2, 5, 6, 2)), dict(warp=torch.zeros(2, 5, 6, 4, dtype=torch.float64)), dict(warp=torch.zeros(5, 4)),
                dict(warp=torch.zeros(2, 0, 6, 4)), dict(image=torch.zeros(2, 4, 4, 7)), dict(image=torch.zeros(3, 3, 4, 7)),
                dict(image=torch.zeros(3, 4, 7)), dict(image=torch.zeros(2, 3, 4, 7, dtype=torch.float16)),
                dict(image=torch.zeros(2, 3, 4, 7, dtype=torch.uint8)), dict(image=torch.zeros(2, 4, 7, 4, dtype=torch.uint8)),
                dict(ts=[]), dict(ts=np.zeros((2, 2))), dict(ts=torch.zeros(2, 2)), dict(certainty=torch.zeros(2, 5, 7)),
                dict(certainty=torch.zeros(5, 6)), dict(certainty=torch.zeros(2, 5, 6, dtype=torch.float64)), dict(dtype=torch.float16),
                dict(background=float("nan"))):
        kw = {**a, **bad}
        with pytest.raises(ValueError):
            roma_amd.render_morph(kw.pop("warp"), kw.pop("image"), kw.pop("ts"), **kw)
    with pytest.raises(TypeError):
        roma_amd.render_morph(np.zeros((5, 6, 4), dtype=np.float32), a["image"], a["ts"])
    with pytest.raises(TypeError):
        roma_amd.render_morph(a["warp"], a["image"], a["ts"], certainty=np.zeros((2, 5, 6), dtype=np.float32))
    # host tensors are refused: there is no CPU path
    calls = (lambda: roma_amd.render_morph(a["warp"], a["image"], a["ts"]),
             lambda: roma_amd.render_morph(a["warp"][0], a["image"][0], roma_amd.morph_times(3), dtype=torch.float32),
             lambda: roma_amd.render_morph(a["warp"], torch.zeros(2, 4, 7, 3, dtype=torch.uint8), np.array([0.25]), certainty=torch.zeros(2, 5, 6)),
             lambda: RegressionMatcher.__new__(RegressionMatcher).render_morph(a["warp"], a["image"], a["ts"], background=0.0),
             lambda: TinyRoMa.__new__(TinyRoMa).render_morph(a["warp"], a["image"], a["ts"]))
    for fn in calls:
        with pytest.raises(_lib.RomaHipError, match="no CPU fallback"):
            fn()


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_morph_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "morph.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/morph.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["morph_pack_kernel"] + [f"render_morph_kernel<{a}, {b}>" for a in ("false", "true") for b in ("false", "true")], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
