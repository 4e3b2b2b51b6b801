"""libroma_hip_f16.so - the same sources built for IEEE binary16 storage (amp_dtype=torch.float16, the reference's default
precision policy: model_zoo/__init__.py:37, matcher.py:46,341, encoders.py:7) - operator parity on MI355X.

Every format-specific piece of the library (conversions, packing, v_mfma_f32_32x32x16_f16, v_dot2_f32_f16) sits in
csrc/common.h; these tests run one operator of every kernel family through the f16 library against torch f64 on the same
f16-rounded operands, with bounds 8 x tighter than the bf16 ones (11 significand bits instead of 8).  The model-level gates
are tests/test_gpu_parity.py::test_h16_tiny_stagewise_vs_oracle[f16] and ::test_f16_full8_vs_reference_golden.

Every roma_op_* entry the `mixed` step reaches with binary16 activations, from the hand-over of the DINOv2 features to the last
refiner_out (plus the VGG front end), and the test here that calls it through lib16.  Bodies named *_case live in
tests/test_gpu_ops.py, where the bfloat16 tests run them with divisor 1; here every 16-bit bound is the bfloat16 one / 8.

  roma_op_convert_from_bf16                     test_convert_from_bf16_is_torch_half
  roma_op_conv3x3 / _c3_bf16                    test_conv3x3_f16, test_conv1_1_from_f32_image_f16
  roma_op_maxpool2x2, roma_op_pool_proj         test_pool_proj_f16
  roma_op_gemm   f16 -> f16, bias, activation   test_gemm_f16 (also the proj heads and the decoder's fc1 + GELU)
                 f16 -> f32, bias               test_gemm_f16 (the decoder's to_out)
                 f16 -> f32 + f32 residual      test_decoder_gemm_f32_residual_in_place_f16
                 subnormal operands             test_gemm_subnormal_operands_f16
  roma_op_gemm_res_bf16 (--dtype f16 only)      test_gemm_f16_residual_in_place
  roma_op_gp                                    test_gp_posterior_f16_features_vs_oracle
  roma_op_layernorm, roma_op_layernorm_dt       test_layernorm_f16
  roma_op_qkv_scatter_gemm, roma_op_attention   test_attention_f16, test_attention_deferred_rescale_f16,
                                                test_attention_deferred_rescale_top_of_range_v_f16,
                                                test_attention_ignores_padding_rows_f16
  roma_op_refiner_input                         test_refiner_input_f16
  roma_op_local_corr_window                     test_local_corr_window_f16, test_local_corr_subnormal_operands_f16
  roma_op_dwconv5x5                             test_dwconv5x5_f16, test_refiner_wide_pair_f16 (with the 1x1 as a GEMM)
  roma_op_refiner_block                         test_refiner_block_f16
  roma_op_refiner_block_final, _apply_delta     test_refiner_block_final_f16
  roma_op_refiner_out                           test_refiner_out_f16
(roma_op_cls_to_flow and roma_op_resize_bilinear are f32 in both libraries: tests/test_gpu_ops.py.)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops as ops
from test_gpu_ops import Fmt, P, ok, rnd

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope="module")
def lib16(built_lib):
    from roma_amd import _lib
    lib = _lib.load("f16")
    assert lib.roma_h16_format() == F16 and b"f16" in lib.roma_version()
    return lib


@pytest.fixture(scope="module")
def f16(lib16):
    """binary16 for the shared test bodies: 11 significand bits against bfloat16's 8, so every 16-bit bound is divided by 8"""
    return Fmt(lib16, F16, torch.float16, 8.0)


def test_each_library_rejects_the_other_16_bit_code(built_lib, lib16):
    """The 16-bit format is a build property: the other code is an error, never a reinterpretation of the bits."""
    a = torch.zeros(64, 64, device="cuda", dtype=torch.float16)
    o = torch.zeros(64, 64, device="cuda", dtype=torch.float16)
    for lib, bad in ((lib16, BF16), (built_lib, F16)):
        rc = lib.roma_op_gemm(P(a), 64, P(a), 64, P(o), 64, 64, 64, 64, 1, 0, 0, 0, None, None, None, 0, 0, 1.0, bad, bad, None)
        assert rc != 0 and b"this library stores" in lib.roma_last_error()
    from roma_amd import _lib
    cfg = _lib.RomaConfig(112, 112, 0, 0, 1, 0, 1, BF16, 1, 0)
    h = C.c_void_p()
    assert lib16.roma_create(C.byref(cfg), C.byref(h)) != 0


@pytest.mark.parametrize("M,N,K,act", [(300, 200, 72, 0), (2500, 144, 144, 1), (9000, 768, 1024, 2), (25616, 1024, 1024, 0),
                                       (70000, 576, 576, 1), (8300, 1152, 1152, 0), (512, 1024, 4096, 0)])
def test_gemm_f16(lib16, M, N, K, act):
    """classic / 8-phase / 6-phase kernels: f16 in, f32 and f16 out, bias + activation"""
    A, W, b = rnd(M, K, seed=1).half(), rnd(N, K, seed=2, std=K ** -0.5).half(), rnd(N, seed=3)
    ref = A.double() @ W.double().T + b.double()
    ref = F.relu(ref) if act == 1 else (F.gelu(ref) if act == 2 else ref)
    Ad, Wd, bd = A.cuda(), W.cuda(), b.cuda()
    for dt_out, tdt, tol in ((F32, torch.float32, 2e-4), (F16, torch.float16, 2.5e-3)):
        out = torch.empty((M, N), device="cuda", dtype=tdt)
        ok(lib16, lib16.roma_op_gemm(P(Ad), K, P(Wd), K, P(out), N, M, N, K, 1, 0, 0, 0, P(bd), None, None, 0, act, 1.0, F16, dt_out, None))
        torch.cuda.synchronize()
        err = (out.cpu().double() - ref).abs()
        assert bool((err <= tol * (1.0 + ref.abs())).all()), (dt_out, float(err.max()))


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 70, 70, 256, 512), (2, 72, 70, 64, 64), (2, 36, 40, 64, 128), (1, 54, 54, 128, 128)])
def test_conv3x3_f16(lib16, B, H, W, Cin, Cout):
    """implicit-GEMM 3x3 (gemm8p) and the weight-stationary front-end kernels (conv64.hip) in f16"""
    x, w, b = rnd(B, Cin, H, W, seed=1).half(), rnd(Cout, Cin, 3, 3, seed=2, std=(9 * Cin) ** -0.5).half(), rnd(Cout, seed=3)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    xin = x.permute(0, 2, 3, 1).contiguous().cuda()
    wp = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().cuda()
    out = torch.zeros((B, H, W, Cout), device="cuda", dtype=torch.float16)
    ok(lib16, lib16.roma_op_conv3x3(P(xin), P(wp), P(b.cuda()), P(out), B, H, W, Cin, Cout, 1, F16, None))
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= 2.5e-3 * (1.0 + ref.abs())).all()), float(err.max())


def test_conv1_1_from_f32_image_f16(lib16):
    B, H, W = 2, 40, 56
    x, w, b = rnd(B, 3, H, W, seed=1), rnd(64, 3, 3, 3, seed=2, std=0.2).half(), rnd(64, seed=3)
    ref = F.relu(F.conv2d(x.half().double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    wp = torch.zeros(64, 32, dtype=torch.float16)
    wp[:, :27] = w.reshape(64, 27)
    out = torch.zeros((B, H, W, 64), device="cuda", dtype=torch.float16)
    ok(lib16, lib16.roma_op_conv3x3_c3_bf16(P(x.cuda()), P(wp.cuda()), P(b.cuda()), P(out), B, H, W, None))
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= 2.5e-3 * (1.0 + ref.abs())).all()), float(err.max())


@pytest.mark.parametrize("Cp,B,H,W", [(576, 2, 40, 36), (1152, 1, 27, 30)])
def test_dwconv5x5_f16(lib16, Cp, B, H, W):
    x, w, b = rnd(B, Cp, H, W, seed=1).half(), rnd(Cp, 1, 5, 5, seed=2, std=0.2), rnd(Cp, seed=3)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=2, groups=Cp)).permute(0, 2, 3, 1)
    wp = w.reshape(Cp, 25).T.contiguous().cuda()
    xin = x.permute(0, 2, 3, 1).contiguous().cuda()
    outs = []
    try:
        for mode in (0, 2):  # register-prefetch kernel / wave-private ring kernel (dwconv_ring.hip): bit-identical
            lib16.roma_tuning(b"dw_ring", mode)
            out = torch.full((B, H, W, Cp), float("nan"), device="cuda", dtype=torch.float16)
            ok(lib16, lib16.roma_op_dwconv5x5(P(xin), P(out), P(wp), P(b.cuda()), B, H, W, Cp, F16, None))
            torch.cuda.synchronize()
            outs.append(out)
    finally:
        lib16.roma_tuning(b"dw_ring", -1)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    err = (outs[1].cpu().double() - ref).abs()
    assert bool((err <= 2.5e-3 * (1.0 + ref.abs())).all()), float(err.max())


@pytest.mark.parametrize("Cp,B,H,W", [(24, 1, 75, 301), (144, 1, 41, 59), (144, 2, 70, 280)])
def test_refiner_block_f16(lib16, Cp, B, H, W):
    x = rnd(B, Cp, H, W, seed=1).half()
    w, b = rnd(Cp, 1, 5, 5, seed=2, std=0.2), rnd(Cp, seed=3)
    pw, pb = rnd(Cp, Cp, seed=4, std=Cp ** -0.5).half(), rnd(Cp, seed=5)
    mid = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=2, groups=Cp)).half()
    ref = (F.conv2d(mid.double(), pw.double()[:, :, None, None], pb.double())).permute(0, 2, 3, 1)
    out = torch.full((B, H, W, Cp), float("nan"), device="cuda", dtype=torch.float16)
    wp = w.reshape(Cp, 25).T.contiguous().cuda()
    xin = x.permute(0, 2, 3, 1).contiguous().cuda()
    ok(lib16, lib16.roma_op_refiner_block(P(xin), P(out), P(wp), P(b.cuda()), P(pw.cuda()), P(pb.cuda()), B, H, W, Cp, F16, None))
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    # f16 output rounding (2^-11 relative) + the occasional 1-ulp flip of the f16 intermediate
    assert bool((err <= 2e-3 * ref.abs() + 5e-3).all()), float(err.max())
    assert float(err.mean()) < 1e-3


@pytest.mark.parametrize("r,c,h,w", [(2, 256, 37, 43), (3, 512, 35, 35), (7, 512, 20, 24)])
def test_local_corr_window_f16(lib16, r, c, h, w):
    """tile + work-list kernels (v_dot2_f32_f16) through the Python operator boundary (float16 tensors select the f16
    library) against the oracle on f16-rounded features: smooth field, an incoherent band, far-outside targets."""
    from oracle import roma_oracle
    from roma_amd.local_correlation import local_correlation
    B = 2
    f0, f1 = rnd(B, c, h, w, seed=1), rnd(B, c, h, w, seed=2)
    warp = roma_oracle.pixel_grid(B, h, w) * 1.15 + 0.08 + rnd(B, 2, h, w, seed=3, std=0.004)
    warp[:, :, h // 2:h // 2 + 5] += rnd(B, 2, 5, w, seed=4, std=0.5)
    warp[1, :, :3, :3] = 3.0
    ref = roma_oracle.local_correlation(f0.half().float(), f1.half().float(), r, warp)
    out = local_correlation(f0.cuda().half(), f1.cuda().half(), r, warp.cuda())
    assert torch.allclose(out.cpu(), ref, atol=2e-4, rtol=1e-4), float((out.cpu() - ref).abs().max())


# ------------------------------------------------------------------ the decoder, GP and refiner ends in binary16
@pytest.mark.parametrize("B,heads,hd,N", [(2, 8, 128, 64),      # one key tile
                                          (1, 8, 128, 200),     # 4 tiles: both LDS buffer instances as non-first tiles, masked tail
                                          (2, 8, 128, 321),     # the last tile has one valid key
                                          (1, 3, 64, 40),
                                          (2, 2, 64, 128),      # no masked tile
                                          (5, 2, 128, 1700)])   # B N >= 8192 rows: the persistent QKV epilogue
def test_attention_f16(f16, B, heads, hd, N):
    """roma_op_qkv_scatter_gemm + roma_op_attention (the decoder's form: 8 heads of 128) against an f64 softmax of the same
    f16-rounded x and w: scatter layout to 3e-2 / 8, output to 6e-2 / 8.  A torch emulation of the design (q, k, v and P rounded
    to f16, f32 row sums, f16 output) deviates from the f64 reference by at most 4.1e-3 on these six cases (bound 7.5e-3); the
    largest |k| is 9.0 (the 1700-token case), its rounding 3.5e-3 (bound 3.75e-3)."""
    ops._attention_case(f16, B, heads, hd, N)


RESCALE_SHAPES = [(128, 200), (128, 321), (64, 40), (64, 200)]


@pytest.mark.parametrize("hd,N", RESCALE_SHAPES)
def test_attention_deferred_rescale_f16(f16, hd, N):
    """tests/test_gpu_ops.py::test_attention_deferred_rescale in binary16, where the limit 2^14 of the deferred rescale is what
    keeps P inside the format: the late key beats the earlier tiles by more than e^12 in both directions and by more than e^89
    for some queries (measured: 140 - 175), against an f64 softmax to 3e-2 / 8 = 3.75e-3.  The design emulated in torch (P
    relative to the row maximum rounded to f16, f32 row sum, f16 output) deviates by 1.0e-3.  Defects emulated in torch on the
    same operands (reference = maximum of tile 0, never moved), N > 64:
      * P clipped at 65504 when it is packed, the f32 row sum unclipped: error 2.8 - 3.7, 750 - 980 x the bound (with the row
        sum taken from the clipped P as well the error is only 1 - 2 x the bound: that variant is not what this test is for);
      * P stored in f16 at that reference: 417 - 694 values of P are +inf, a third of the outputs are not finite."""
    ops.deferred_rescale_case(f16, hd, N, top_jump=89.0 if N > 64 else None)


@pytest.mark.parametrize("hd,N", RESCALE_SHAPES)
def test_attention_deferred_rescale_top_of_range_v_f16(f16, hd, N):
    """The same forced late key with every tenth column of V at +-60000: a stale reference puts P up to 2^14 next to |V| at the
    top of binary16's range, and only the f32 accumulator may see the product.  The output must be finite and inside the bound
    of the test above scaled by max |v| / 4 of the column (every error term is linear in V): 56 for the big columns, where one
    f16 ulp is 32.  Design emulation as above: 0.33 of the bound.  Defect emulated in torch: P V formed in f16 before it is
    accumulated - 3 600 to 12 700 products per case are not finite."""
    ops.deferred_rescale_case(f16, hd, N, big_v=True)


@pytest.mark.parametrize("hd,N", RESCALE_SHAPES)
def test_attention_ignores_padding_rows_f16(f16, hd, N):
    """tests/test_gpu_ops.py::test_attention_ignores_padding_rows in binary16: bit-identical outputs whatever rows N .. Npad
    hold.  Defect emulated in torch (a padding query's vote moves the reference of its wave at tile 1, which re-rounds the P of
    the wave's valid queries): 47 - 54 % of the outputs of the wave that holds valid and padding queries change bits, against a
    bound of none.  (64, 40) has one key tile, where no vote is taken: it checks the masking alone."""
    ops.padding_rows_case(f16, hd, N)


@pytest.mark.parametrize("in16", [False, True])
@pytest.mark.parametrize("M", [5, 1603])
def test_layernorm_f16(f16, M, in16):
    """f32 -> f16 (the decoder blocks: f32 token stream) and f16 -> f16; f16 in with f32 out stays refused"""
    ops.layernorm_case(f16, M, in16)


@pytest.mark.parametrize("M,N,K", [(300, 64, 72), (8229, 640, 192)])
def test_decoder_gemm_f32_residual_in_place_f16(lib16, M, N, K):
    """The decoder blocks' proj / fc2 form: f16 in, f32 out, bias, per-column scale and an f32 residual updated in place (small
    4-wave tiles; the persistent 8-wave kernel with a ragged last m-tile and a partial n-tile).  f32-level bound of
    test_gemm_f16's f32 output."""
    A, W, b = rnd(M, K, seed=1).half(), rnd(N, K, seed=2, std=K ** -0.5).half(), rnd(N, seed=3)
    s, r = rnd(N, seed=4), rnd(M, N, seed=5)
    ref = (A.double() @ W.double().T + b.double()) * s.double() + r.double()
    x = r.clone().cuda()
    ok(lib16, lib16.roma_op_gemm(P(A.cuda()), K, P(W.cuda()), K, P(x), N, M, N, K, 1, 0, 0, 0, P(b.cuda()), P(s.cuda()), P(x), N, 0, 1.0,
                                 F16, F32, None))
    torch.cuda.synchronize()
    err = (x.cpu().double() - ref).abs()
    assert bool((err <= 2e-4 * (1.0 + ref.abs())).all()), float(err.max())


@pytest.mark.parametrize("M,N,K", [(300, 64, 72), (1000, 1024, 512)])
def test_gemm_f16_residual_in_place(f16, M, N, K):
    """roma_op_gemm_res_bf16 of the f16 library (--dtype f16: the f16 residual stream of DINOv2): one rounding of the branch plus
    one of the sum, 2^-11 each; N % 8 != 0 refused"""
    ops.gemm_residual_in_place_case(f16, M, N, K)


@pytest.mark.parametrize("b,h,w", ops.GP_SHAPES)
def test_gp_posterior_f16_features_vs_oracle(f16, b, h, w):
    """roma_op_gp from f16 features against the oracle on the same rounded features, under the f32 bound (see
    tests/test_gpu_ops.py::test_gp_posterior_vs_oracle)"""
    ops.gp_case(f16, b, h, w)


@pytest.mark.parametrize("C,E,K,ldf,ldd,h,w", [(512, 64, 49, 512, 1152, 21, 19), (256, 32, 25, 256, 576, 30, 28),
                                               (64, 16, 0, 64, 144, 33, 40), (9, 6, 0, 16, 24, 50, 47)])
def test_refiner_input_f16(f16, C, E, K, ldf, ldd, h, w):
    ops.refiner_input_case(f16, C, E, K, ldf, ldd, h, w)


@pytest.mark.parametrize("Cp,M", [(24, 255), (24, 4099), (144, 4099), (576, 1027)])
def test_refiner_out_f16(f16, Cp, M):
    """the lane-per-row kernel (Cp = 24) and the shared-row kernels on f16 rows; f32-level bounds"""
    ops.refiner_out_case(f16, Cp, M)


@pytest.mark.parametrize("B,H,W", [(2, 13, 10), (2, 1, 30), (1, 75, 3), (1, 41, 59)])
def test_refiner_wide_pair_f16(f16, B, H, W):
    """The C = 576 block as the model runs it (dwconv5x5, then the 1x1 as a GEMM) in f16, under the bounds of
    tests/test_gpu_ops.py::test_refiner_wide_pair_vs_f64 / 8.  A torch emulation of the pair on the CPU (f32 depthwise rounded to
    f16, f32 matmul rounded to f16) stays inside them on all four shapes: worst error / bound 0.22, worst mean error 1.9e-4
    (bound 7.5e-4), 99.97 % of the stencil outputs bit-equal to the once-rounded f64 ones."""
    ops.refiner_wide_pair_case(f16, B, H, W)


@pytest.mark.parametrize("Cp,B,H,W", [(24, 2, 13, 10), (24, 3, 3, 200), (144, 2, 13, 10), (144, 2, 1, 30), (144, 1, 41, 59)])
def test_refiner_block_final_f16(f16, Cp, B, H, W):
    """roma_op_refiner_block_final + roma_op_refiner_apply_delta in f16.  With weights of scale Cp^-0.5 the 16-bit remainder of
    the composed weights is about 2^-12 |w|: below 2^-14, a SUBNORMAL f16, for 98.8 % of the entries at Cp = 144 (93 % at 24;
    asserted: more than half) - the f32-level bound 2e-5 holds only if the matrix core honours subnormal f16 operands.  Defect
    emulated in torch (subnormal remainders flushed to zero): error 3.5e-4 - 7.2e-4 = 5.0 - 8.1 x the bound at Cp = 144 (3.8
    and 4.1 x at Cp = 24); the design (f32 sums of head and remainder products) deviates by 8e-7."""
    ops.refiner_block_final_case(f16, Cp, B, H, W, subnormal_share=0.5)


@pytest.mark.parametrize("C,N,ldf", [(64, 9, 16), (128, 64, 64)])
@pytest.mark.parametrize("B,H,W", [(1, 9, 33), (3, 37, 70)])
def test_pool_proj_f16(f16, C, N, ldf, B, H, W):
    """roma_op_pool_proj bit-identical to roma_op_maxpool2x2 + roma_op_gemm, the pooled map bit-equal to F.max_pool2d"""
    ops.pool_proj_case(f16, C, N, ldf, B, H, W)


# bfloat16 values the hand-over must get right: signed zeros; 65280 (the largest bfloat16 below binary16's overflow point
# 65520, exact in f16) and 65536 (the first above: +-inf); huge and infinite; NaN; [2^-25, 2^-14]: 2^-25 is the tie between 0
# and the smallest subnormal (to even: 0), 1.5 x 2^-24 the tie between 2^-24 and 2^-23 (to even: 2^-23), 2^-14 the smallest
# normal number; 2^-26 vanishes
CONVERT_SPECIALS = [0.0, -0.0, 65280.0, 65536.0, -65280.0, -65536.0, 65024.0, 66048.0, 3e38, -3e38, float("inf"), float("-inf"),
                    float("nan"), 2.0 ** -25, -2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24, -1.5 * 2.0 ** -24,
                    1.25 * 2.0 ** -24, 1.75 * 2.0 ** -23, 2.0 ** -14, 2.0 ** -26, 0.999 * 2.0 ** -14]


@pytest.mark.parametrize("n", [4, 1028, 4 * (65536 * 256 + 3)])
def test_convert_from_bf16_is_torch_half(lib16, n):
    """roma_op_convert_from_bf16 - the one kernel between the bfloat16 DINOv2 and the binary16 decoder of `mixed` - is bit for
    bit x.float().half(): overflow to inf, gradual underflow with ties to even.  n = 4 (65280, 65536, -0.0, 1.5 x 2^-24);
    1028; 4 (65536 x 256 + 3): the first size at which the grid-stride loop makes a second trip (its 12 elements are specials).
    Random values span 2^-30 .. 2^18: 33 of the 1028 and 2.4 M of the 67 M overflow, 235 and 15 M are subnormal.  Defect
    emulated in torch (the input clamped to +-65504 first): 7 of the 24 specials and every one of those overflowing random
    values differ in bits, against a bound of none."""
    spec = torch.tensor(CONVERT_SPECIALS).bfloat16()
    # the specials are what the comment above says once they are bfloat16, and the reference treats them as it says
    assert spec[[2, 3, 13, 17]].float().tolist() == [65280.0, 65536.0, 2.0 ** -25, 1.5 * 2.0 ** -24]
    assert spec[[2, 3, 13, 17]].float().half().float().tolist() == [65280.0, float("inf"), 0.0, 2.0 ** -23]
    if n == 4:
        x = spec[[2, 3, 1, 17]].clone()
    else:
        g = torch.Generator().manual_seed(3)
        x = (torch.randn(n, generator=g) * torch.exp2((torch.arange(n) % 49 - 30).float())).bfloat16()
        x[:24], x[-24:] = spec, spec
    ref = x.float().half()
    assert bool(torch.isinf(ref).any()) and bool(((ref != 0) & (ref.float().abs() < 2.0 ** -14)).any())
    out = torch.full((n,), 7.0, device="cuda", dtype=torch.float16)
    ok(lib16, lib16.roma_op_convert_from_bf16(P(x.cuda()), P(out), n, None))
    torch.cuda.synchronize()
    got = out.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    bits, rbits = got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan]
    assert torch.equal(bits, rbits), int((bits != rbits).sum())
    assert lib16.roma_op_convert_from_bf16(P(x.cuda()), P(out), 6, None) != 0
    assert lib16.roma_op_convert_from_bf16(P(x.cuda()), P(out), 0, None) != 0


@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (300, 200, 72)])
def test_gemm_subnormal_operands_f16(lib16, M, N, K):
    """v_mfma_f32_32x32x16_f16 with SUBNORMAL f16 operands: A = randn x 2^-20 is wholly below 2^-14 once rounded, W = randn x 2^10;
    f64 on the rounded operands, test_gemm_f16's f32-output bound scaled by the output's own magnitude.  A matrix core that
    flushed subnormal operands would return zeros: an error of max |ref|, 2 500 x the bound."""
    A, W = (rnd(M, K, seed=1) * 2.0 ** -20).half(), (rnd(N, K, seed=2) * 2.0 ** 10).half()
    assert float(A.float().abs().max()) < 2.0 ** -14 and float((A != 0).float().mean()) > 0.9
    ref = A.double() @ W.double().T
    scale = float(ref.abs().max())
    out = torch.full((M, N), float("nan"), device="cuda")
    ok(lib16, lib16.roma_op_gemm(P(A.cuda()), K, P(W.cuda()), K, P(out), N, M, N, K, 1, 0, 0, 0, None, None, None, 0, 0, 1.0, F16, F32, None))
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs()
    print(f"gemm, subnormal f16 A ({M}, {N}, {K}): max |out - f64| = {float(err.max()):.2e}, max |ref| = {scale:.2e}")
    assert bool((err <= 2e-4 * (scale + ref.abs())).all()), (float(err.max()), scale)


def test_local_corr_subnormal_operands_f16(lib16):
    """The (19, 21) "uniform" case of tests/test_gpu_lc_sort.py at r = 2 with f0 x 2^-18 (subnormal in f16) and f1 x 2^8: the sorted
    items on the matrix core (lc_bin 1) and the per-query packed dot v_dot2_f32_f16 (lc_bin 0) must agree within 2e-5 / 1e-5 as
    they do on normal numbers, and both must match f64 on the rounded operands within test_local_corr_window_f16's bound at
    this output's magnitude (2e-4 at max |out| = 4, i.e. 5e-5 max |ref|; rtol 1e-4).  Outputs are about 1e-3: a path that
    flushed subnormal operands would return zeros, 50 x the first bound and 20 x the second."""
    from oracle import roma_oracle
    from test_gpu_lc_sort import B, CH, _warp
    h, w, r = 19, 21, 2
    K = (2 * r + 1) ** 2
    g = np.random.Generator(np.random.PCG64(7 + h * 64 + w))
    f0 = (torch.from_numpy(g.standard_normal(size=(B, h * w, CH), dtype=np.float32)) * 2.0 ** -18).half()
    f1 = (torch.from_numpy(g.standard_normal(size=(B, h * w, CH), dtype=np.float32)) * 2.0 ** 8).half()
    warp = _warp("uniform", h, w)
    assert float(((f0 != 0) & (f0.float().abs() < 2.0 ** -14)).float().mean()) > 0.9
    nchw = lambda t: t.double().reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous()
    ref = roma_oracle.local_correlation(nchw(f0), nchw(f1), r, nchw(warp)).reshape(B, K, h * w).permute(0, 2, 1)
    scale = float(ref.abs().max())
    f0d, f1d, wd = f0.cuda(), f1.cuda(), warp.cuda()
    outs = {}
    try:
        assert lib16.roma_tuning(b"lc_mode", 1) == 0   # every tile on the incoherent list (see test_gpu_lc_sort.py)
        for binned in (1, 0):
            assert lib16.roma_tuning(b"lc_bin", binned) == 0
            out = torch.full((B, h * w, K), float("nan"), device="cuda")
            ok(lib16, lib16.roma_op_local_corr_window(P(f0d), P(f1d), P(wd), P(out), B, h, w, CH, r, CH ** -0.5, K, F16, F32, None))
            torch.cuda.synchronize()
            outs[binned] = out.cpu().double()
    finally:
        lib16.roma_tuning(b"lc_bin", -1)
        lib16.roma_tuning(b"lc_mode", -1)
    for binned, o in outs.items():
        err = (o - ref).abs()
        print(f"local_corr, subnormal f16 f0, lc_bin {binned}: max |out - f64| = {float(err.max()):.2e}, max |ref| = {scale:.2e}")
    assert scale > 5e-4
    assert np.allclose(outs[1].numpy(), outs[0].numpy(), atol=2e-5, rtol=1e-5), float((outs[1] - outs[0]).abs().max())
    for binned, o in outs.items():
        assert bool(((o - ref).abs() <= 5e-5 * scale + 1e-4 * ref.abs()).all()), (binned, float((o - ref).abs().max()), scale)
