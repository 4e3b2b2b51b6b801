"""Every operator writes its own output and nothing else (MI355X, both 16-bit libraries).

The parity tests allocate each output at exactly the operator's size; the caching allocator rounds that up, so a store a few
elements past the end, or into the pad columns of a strided row, passes them.  Here every output and every activation input
lives in a guarded buffer (tests/extents_cases.py): 4 KiB of 0xFF bytes - NaN in every floating format - on either side.
  (a) after the launch the guards of every buffer are bit-intact;
  (b) the inputs' guards are NaN, so a halo or tail read that leaks into a result makes it non-finite;
  (c) where an entry takes a leading dimension it gets a padded one, and the pad has its documented fate (include/roma_hip.h):
      untouched for roma_op_gemm (ldc > N), roma_op_gemm_res_bf16, roma_op_local_corr_window (ldo > K) and the Kcorr slice of
      roma_op_refiner_input; zero for the tail of roma_op_refiner_input, the columns [N, ldf) of roma_op_pool_proj and the rows
      [N, npad) of the attention workspaces;
  (d) the values are held to the reference and the bound that the operator's parity test already uses (the *_case bodies of
      tests/test_gpu_ops.py with the guarded allocator, or the same reference and bound restated here).
Which kernel ran is asserted through roma_profile_report where the launcher names it, else through the roma_tuning switch that
selects it.  Ordinary launches on valid shapes: nothing here is meant to fault, nothing runs in a loop."""
import contextlib
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops as ops
import tiny_ops_cases as tc
from conftest import GOLDEN, ROOT
from extents_cases import Guarded, assert_columns
from test_gpu_f16 import f16, lib16  # noqa: F401  (fixtures: the binary16 library and its format)
from test_gpu_ops import Fmt, P, ok, rnd
from test_gpu_tuning import run_child

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope="module", params=["bf16", "f16"])
def f(request, built_lib):
    """the 16-bit format of each library, as the shared case bodies take it"""
    assert torch.cuda.is_available()
    if request.param == "bf16":
        return ops.fmt_of(built_lib, BF16)
    return request.getfixturevalue("f16")


def f32_of(f):
    return Fmt(f.lib, F32, torch.float32, 1.0)


def fmt_for(f, dt):
    return f32_of(f) if dt == F32 else f


def h16(f):
    return "bf16" if f.dt == BF16 else "f16"


def dtn(f, dt):
    return "f32" if dt == F32 else h16(f)


@contextlib.contextmanager
def kernels_of(lib):
    """the names under which the launches inside the block were profiled (roma_profile_report), filled in at its end"""
    names = []
    ok(lib, lib.roma_profile_enable(1))
    try:
        yield names
        torch.cuda.synchronize()
        n = lib.roma_profile_report(None, 0)
        buf = C.create_string_buffer(int(n))
        assert lib.roma_profile_report(buf, n) > 0
        names.extend(sorted(json.loads(buf.value.decode())))
    finally:
        lib.roma_profile_enable(0)


@contextlib.contextmanager
def tuned(lib, **switches):
    try:
        for key, value in switches.items():
            ok(lib, lib.roma_tuning(key.encode(), value))
        yield
    finally:
        for key in switches:
            lib.roma_tuning(key.encode(), -1)


def finite(t):
    return bool(torch.isfinite(t.float()).all())


# ================================================================================================ pool_proj
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (2, 5, 33), (1, 9, 70)])
@pytest.mark.parametrize("Cc,N,ldf", [(64, 8, 8), (64, 9, 16), (64, 20, 24), (64, 32, 32),
                                      (128, 33, 40), (128, 40, 48), (128, 50, 56), (128, 64, 64)])
def test_pool_proj(f, Cc, N, ldf, B, H, W):
    """Every ldf that pool_proj_supported accepts, ldf % 16 == 8 included: there the second half-wave of the last column pair
    has no columns of its own - its store would land in the next pixel's first eight outputs, and behind the last pixel in the
    16 bytes past the end of pf.  Minimum size, an odd H whose last row has no partner, a ragged 32-pixel column tile, several
    column tiles.  Zeros in [N, ldf) (roma_hip.h), bit-identity with maxpool2x2 + gemm (asserted by the case)."""
    al = Guarded()
    with kernels_of(f.lib) as ran:
        pf, pooled = ops.pool_proj_case(f, Cc, N, ldf, B, H, W, alloc=al)
    assert "pool_proj_kernel<%d>" % Cc in ran, ran
    assert_columns(pf, N, ldf, "zero", "pf")
    assert finite(pf) and finite(pooled)


# ================================================================================================ gemm
def gemm_close(f, dt_in, dt_out, got, ref, K):
    """the bounds of the parity tests: test_gemm_f32_epilogues; test_gemm_big_m_bf16 / test_gemm8p_matches_classic_and_reference
    (W of standard deviation K^-1/2); test_gemm_f16"""
    err = (got.cpu().double() - ref).abs()
    if dt_in == F32:
        bound = 2e-4 * math.sqrt(K) + 1e-5 * ref.abs()
    elif f.dt == BF16:
        atol, rtol = (2e-3, 1e-4) if dt_out == F32 else (0.03, 1e-2)
        bound = atol + rtol * ref.abs()
    else:
        bound = (2e-4 if dt_out == F32 else 2.5e-3) * (1.0 + ref.abs())
    assert bool((err <= bound).all()), float((err - bound).max())  # (a NaN compares false)


def gemm_guarded(f, dt_in, dt_out, M, N, K, kernel, act=0, batch=1, gap_rows=0, pad=8, **switches):
    """out[batch][M + gap_rows][N + pad]: the rows [M, M + gap_rows) lie between the items (sC > M ldc), the columns [N, N + pad)
    behind every row; both must come back untouched, the guards intact, the values within the operator's bound"""
    lib = f.lib
    tin, tout = fmt_for(f, dt_in).tdt, fmt_for(f, dt_out).tdt
    A, W, b = rnd(batch, M, K, seed=1).to(tin), rnd(N, K, seed=2, std=K ** -0.5).to(tin), rnd(N, seed=3)
    # the f64 reference on every row, or (the one large problem) on the first, middle and last rows as the parity tests do
    sel = torch.arange(M) if M * N * K < 4e9 else torch.cat([torch.arange(0, 96), torch.arange(M // 2 - 40, M // 2 + 40), torch.arange(M - 96, M)])
    ref = A[:, sel].double() @ W.double().T + b.double()
    ref = F.relu(ref) if act == 1 else ref
    al = Guarded()
    ldc, rows = N + pad, M + gap_rows
    Ad, Wd, bd = al.inp(A), W.cuda(), b.cuda()
    out = al.out((batch, rows, ldc), tout)
    with tuned(lib, **switches), kernels_of(lib) as ran:
        ok(lib, lib.roma_op_gemm(P(Ad), K, P(Wd), K, P(out), ldc, M, N, K, batch, M * K, 0, rows * ldc, P(bd), None, None, 0, act, 1.0,
                                 dt_in, dt_out, None))
    assert ran == [kernel], (ran, kernel)
    al.check()
    assert_columns(out[:, :M], N, ldc, "untouched", "C")
    assert_columns(out[:, M:], 0, ldc if gap_rows else 0, "untouched", "the rows between the items")
    assert finite(out[:, :M, :N])
    gemm_close(f, dt_in, dt_out, out[:, sel.cuda(), :N], ref, K)


# the tile configurations of launch_shape (gemm_kernel.inc) as the profile names them: WM, WN, TM, TN
TILES = {"128x32": "4,1,1,1", "128x64": "4,1,1,2", "128x160": "4,1,1,5", "128x128": "2,2,2,2", "256x64": "8,1,1,2",
         "256x128": "4,2,2,2", "256x192": "4,2,2,3", "256x256": "2,4,4,2"}
# (M, N): the smallest problem launch_shape routes to the tile, with a ragged last m-tile and a ragged last n-tile; K = 24 keeps
# every 16-bit problem off the 8-phase kernels (they ask for K >= 256).  f32 problems with N >= 384 that fill fewer than 192
# tiles of 256 x 256 go to 128 x 128 tiles instead, so the f32 256 x 192 case is wider.
TILE_SHAPES = {"128x32": (130, 24), "128x64": (130, 72), "128x160": (130, 136), "128x128": (2005, 2504), "256x64": (8200, 40),
               "256x128": (8200, 72), "256x192": (8200, 568), "256x256": (8200, 200)}
F32_256x192 = (8200, 1336)


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("pair", ["f32_f32", "h16_h16", "h16_f32"])
def test_gemm_tile_kernels(f, pair, tile):
    dt_in, dt_out = (F32 if pair.startswith("f32") else f.dt), (F32 if pair.endswith("f32") else f.dt)
    M, N = F32_256x192 if (dt_in == F32 and tile == "256x192") else TILE_SHAPES[tile]
    name = "gemm_kernel<%s,%s,%s,dense>" % (dtn(f, dt_in), dtn(f, dt_out), TILES[tile])
    gemm_guarded(f, dt_in, dt_out, M, N, 24, name)


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("which,M,N,K", [("gemm8p", 8200, 248, 256),   # 8 rows in the last m-tile, 248 of 256 columns, the shortest K
                                          ("gemm6p", 8200, 568, 256)])  # 192-column tiles: 184 columns in the last
def test_gemm_phase_kernels(f, which, M, N, K, out_f32):
    dt_out = F32 if out_f32 else f.dt
    name = "%s_kernel<%s,%s,dense,none>" % (which, h16(f), dtn(f, dt_out))
    gemm_guarded(f, f.dt, dt_out, M, N, K, name, gemm8p=1)


def test_gemm_ws1x1(f):
    """the weight-stationary N = K = 576 kernel takes ldc == N only (ws1x1_try_launch), so there are no pad columns to look at:
    the guards around the 65 536 x 576 output and the NaN behind the activation's last chunk are the check"""
    gemm_guarded(f, f.dt, f.dt, 65536, 576, 576, "ws1x1_kernel<%s,relu>" % h16(f), act=1, pad=0, gemm8p=1, ws1x1=1)


@pytest.mark.parametrize("pair", ["f32_f32", "h16_h16", "h16_f32"])
def test_gemm_batched_strided_gaps(f, pair):
    """three items, sC = (M + 3) ldc: the three rows between two items and the pad columns are not the operator's"""
    dt_in, dt_out = (F32 if pair.startswith("f32") else f.dt), (F32 if pair.endswith("f32") else f.dt)
    name = "gemm_kernel<%s,%s,%s,dense>" % (dtn(f, dt_in), dtn(f, dt_out), TILES["128x64"])
    gemm_guarded(f, dt_in, dt_out, 130, 72, 24, name, batch=3, gap_rows=3)


@pytest.mark.parametrize("M,N,K,kernel", [(300, 64, 72, "gemm_kernel<%s,%s,4,1,1,2,dense>"),
                                          (8200, 248, 256, "gemm_kernel<%s,%s,2,4,4,2,dense>")])
def test_gemm_res_in_place(f, M, N, K, kernel):
    """x = x + ls (A W^T + b) in place with ldc = ldr = N + 8: the eight columns behind every row stay as they were.  The entry
    always passes a per-column scale, which keeps it on the tile kernels (gemm8p_try_launch declines a scale): the 4-wave row
    writer and the persistent 256 x 256 tile with 8 rows in its last m-tile."""
    al = Guarded()
    with kernels_of(f.lib) as ran:
        xw = ops.gemm_residual_in_place_case(f, M, N, K, alloc=al, pad=8)
    assert ran == [kernel % (h16(f), h16(f))], ran
    assert_columns(xw, N, N + 8, "untouched", "x")
    assert finite(xw[:, :N])


# ================================================================================================ conv3x3
def conv_close(f, dt, got, ref):
    """test_conv3x3_implicit_gemm (f32, bf16), test_conv3x3_f16"""
    got = got.cpu().double()
    if dt == F32:
        assert torch.allclose(got, ref, atol=2e-4, rtol=2e-4), float((got - ref).abs().max())
    elif f.dt == BF16:
        assert torch.allclose(got, ref, atol=3e-2, rtol=3e-2), float((got - ref).abs().max())
    else:
        err = (got - ref).abs()
        assert bool((err <= 2.5e-3 * (1.0 + ref.abs())).all()), float(err.max())


def conv_guarded(f, dt, B, H, W, Cin, Cout, kernel, slab=False, **switches):
    lib, tdt = f.lib, fmt_for(f, dt).tdt
    x, w, b = rnd(B, Cin, H, W, seed=1).to(tdt), rnd(Cout, Cin, 3, 3, seed=2, std=(9 * Cin) ** -0.5).to(tdt), rnd(Cout, seed=3)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)  # [cout][tap][ci]
    if slab:
        wt = wt.reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3)  # [cout][slab][tap][64]
    wp = wt.reshape(Cout, 9 * Cin).contiguous().cuda()
    al = Guarded()
    xin = al.inp(x.permute(0, 2, 3, 1).contiguous())
    out = al.out((B, H, W, Cout), tdt)
    op = lib.roma_op_conv3x3_slab if slab else lib.roma_op_conv3x3
    with tuned(lib, **switches), kernels_of(lib) as ran:
        ok(lib, op(P(xin), P(wp), P(b.cuda()), P(out), B, H, W, Cin, Cout, 1, dt, None))
    assert len(ran) == 1 and ran[0].startswith(kernel[0]) and ran[0].endswith(kernel[1]), (ran, kernel)
    al.check()
    assert finite(out)
    conv_close(f, dt, out, ref)


def test_conv3x3_implicit_gemm_f32(f):
    conv_guarded(f, F32, 2, 5, 7, 64, 128, ("gemm_kernel<f32,f32,", ",conv3x3>"))


def test_conv3x3_implicit_gemm_h16(f):
    """Cout = 256 in tap-major order is neither conv64's nor the patch kernel's; 70 rows stay below the 8-phase kernel's 8192"""
    conv_guarded(f, f.dt, 2, 5, 7, 64, 256, ("gemm_kernel<%s,%s," % (h16(f), h16(f)), ",conv3x3>"))


def test_conv3x3_gemm8p(f):
    """91 x 91 = 8281 rows: the smallest square image the 8-phase conv form takes, 89 rows in the last m-tile"""
    conv_guarded(f, f.dt, 1, 91, 91, 64, 256, ("gemm8p_kernel<%s,%s,conv3x3,relu>" % (h16(f), h16(f)), ""), gemm8p=1)


def test_conv3x3_patch_resident(f):
    conv_guarded(f, f.dt, 1, 5, 7, 128, 256, ("conv3x3_patch_kernel<%s,relu>" % h16(f), ""), slab=True, conv_patch=1)


@pytest.mark.parametrize("Cin,Cout,kernel", [(64, 64, "conv3x3_c64_kernel<64>"), (64, 128, "conv3x3_c64_kernel<128>"),
                                             (128, 128, "conv3x3_c128_kernel<128>")])
@pytest.mark.parametrize("B,H,W", [(1, 2, 3), (2, 5, 7)])
def test_conv3x3_weight_stationary(f, Cin, Cout, kernel, B, H, W):
    """conv64_try_launch: 16-bit, ReLU, a bias, ldc == Cout, tap-major weights - any image size; images shorter than the ring
    depth and than one strip, narrower than one x tile, odd extents"""
    conv_guarded(f, f.dt, B, H, W, Cin, Cout, (kernel, ""), conv64=7)


@pytest.mark.parametrize("B,H,W", [(1, 3, 33), (2, 9, 5)])
def test_first_conv(f, B, H, W):
    """conv3x3_c3 (f32 out; its launcher has no profile name) and conv3x3_c3_bf16 from a guarded f32 image: the 3x3 halo is read
    just outside the map.  Bounds: test_maxpool_and_first_conv, test_first_conv_bf16_fused, test_conv1_1_from_f32_image_f16."""
    lib = f.lib
    img, w, b = rnd(B, 3, H, W, seed=1), rnd(64, 3, 3, 3, seed=2, std=0.3), rnd(64, seed=3)
    al = Guarded()
    imd = al.inp(img)
    out = al.out((B, H, W, 64), torch.float32)
    wp = w.permute(1, 2, 3, 0).reshape(27, 64).contiguous().cuda()
    ok(lib, lib.roma_op_conv3x3_c3(P(imd), P(wp), P(b.cuda()), P(out), B, H, W, F32, None))
    torch.cuda.synchronize()
    al.check()
    ref = F.relu(F.conv2d(img.double(), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    assert torch.allclose(out.cpu().double(), ref, atol=1e-5, rtol=1e-5)
    wq = w.to(f.tdt)
    ref16 = F.relu(F.conv2d(img.to(f.tdt).double(), wq.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    wp16 = torch.zeros(64, 32, dtype=f.tdt)
    wp16[:, :27] = wq.reshape(64, 27)
    out16 = al.out((B, H, W, 64), f.tdt)
    with tuned(lib, conv64=7), kernels_of(lib) as ran:
        ok(lib, lib.roma_op_conv3x3_c3_bf16(P(imd), P(wp16.cuda()), P(b.cuda()), P(out16), B, H, W, None))
    assert ran == ["conv3x3_c3_bf16_kernel"], ran
    al.check()
    err = (out16.cpu().double() - ref16).abs()
    if f.dt == BF16:
        assert float((err / (ref16.abs() + 1.0)).max()) <= 2.0 ** -8 + 1e-6, float(err.max())
    else:
        assert bool((err <= 2.5e-3 * (1.0 + ref16.abs())).all()), float(err.max())


# ================================================================================================ dwconv5x5
def dwconv_guarded(f, dt, Cp, B, H, W, ring):
    """test_dwconv5x5 (f32, bf16), test_dwconv5x5_f16"""
    lib, tdt = f.lib, fmt_for(f, dt).tdt
    x, w, b = rnd(B, Cp, H, W, seed=1).to(tdt), rnd(Cp, 1, 5, 5, seed=2, std=0.2), rnd(Cp, seed=3)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=2, groups=Cp)).permute(0, 2, 3, 1)
    al = Guarded()
    xin = al.inp(x.permute(0, 2, 3, 1).contiguous())
    out = al.out((B, H, W, Cp), tdt)
    wp = w.reshape(Cp, 25).T.contiguous().cuda()
    with tuned(lib, dw_ring=ring), kernels_of(lib) as ran:
        ok(lib, lib.roma_op_dwconv5x5(P(xin), P(out), P(wp), P(b.cuda()), B, H, W, Cp, dt, None))
    assert ran == ["dwconv5x5_kernel<%s>" % dtn(f, dt)], ran
    al.check()
    got = out.cpu().double()
    if dt == F32 or f.dt == BF16:
        tol = 1e-5 if dt == F32 else 2e-2
        assert torch.allclose(got, ref, atol=tol, rtol=tol), float((got - ref).abs().max())
    else:
        err = (got - ref).abs()
        assert bool((err <= 2.5e-3 * (1.0 + ref.abs())).all()), float(err.max())
    return out


@pytest.mark.parametrize("Cp,B,H,W", [(24, 1, 1, 1), (264, 2, 3, 17), (256, 3, 1, 5)])
@pytest.mark.parametrize("h16_in", [False, True])
def test_dwconv5x5_rolling_window(f, h16_in, Cp, B, H, W):
    """dw_ring = 0: the register-prefetch kernel for every shape (both kernels report under one profile name)"""
    dwconv_guarded(f, f.dt if h16_in else F32, Cp, B, H, W, 0)


@pytest.mark.parametrize("Cp,B,H,W", [(256, 3, 1, 5), (576, 1, 6, 33)])
def test_dwconv5x5_ring(f, Cp, B, H, W):
    """dw_ring = 2: the ring kernel for every shape it takes (16-bit, Cp % 64 == 0, Cp >= 256); bit-identical to the other"""
    ring = dwconv_guarded(f, f.dt, Cp, B, H, W, 2)
    roll = dwconv_guarded(f, f.dt, Cp, B, H, W, 0)
    assert torch.equal(ring.view(torch.int16), roll.view(torch.int16))


# ================================================================================================ refiner blocks
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 3, 21), (1, 37, 33)])
@pytest.mark.parametrize("Cp", [24, 144])
def test_refiner_block(f, Cp, B, H, W):
    """reference and bounds of test_refiner_block_fused (bf16) / test_refiner_block_f16"""
    lib = f.lib
    x = rnd(B, Cp, H, W, seed=1).to(f.tdt)
    w, b = rnd(Cp, 1, 5, 5, seed=2, std=0.2), rnd(Cp, seed=3)
    pw, pb = rnd(Cp, Cp, seed=4, std=Cp ** -0.5).to(f.tdt), rnd(Cp, seed=5)
    mid = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=2, groups=Cp)).to(f.tdt)
    ref = (F.conv2d(mid.double(), pw.double()[:, :, None, None], pb.double())).permute(0, 2, 3, 1)
    al = Guarded()
    xin = al.inp(x.permute(0, 2, 3, 1).contiguous())
    out = al.out((B, H, W, Cp), f.tdt)
    wp = w.reshape(Cp, 25).T.contiguous().cuda()
    with kernels_of(lib) as ran:
        ok(lib, lib.roma_op_refiner_block(P(xin), P(out), P(wp), P(b.cuda()), P(pw.cuda()), P(pb.cuda()), B, H, W, Cp, f.dt, None))
    assert ran == ["refiner_block_kernel<%d>" % Cp], ran
    al.check()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    if f.dt == BF16:
        assert bool((err <= 1e-2 * ref.abs() + 3e-2).all()), float(err.max())
        assert float(err.mean()) < 6e-3
    else:
        assert bool((err <= 2e-3 * ref.abs() + 5e-3).all()), float(err.max())
        assert float(err.mean()) < 1e-3


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 3, 21), (1, 37, 33)])
@pytest.mark.parametrize("Cp", [24, 144])
def test_refiner_block_final(f, Cp, B, H, W):
    """delta [M][4] f32, then the apply pass on guarded flow / certainty"""
    with kernels_of(f.lib) as ran:
        ops.refiner_block_final_case(f, Cp, B, H, W, alloc=Guarded())
    assert "refiner_block_final_kernel<%d>" % Cp in ran, ran


# ================================================================================================ refiner ends
@pytest.mark.parametrize("M", [1, 255, 257])
@pytest.mark.parametrize("Cp,h16_in", [(24, True), (144, True), (576, True), (24, False)])
def test_refiner_out(f, Cp, h16_in, M):
    """the lane-per-row kernel (16-bit, Cp = 24) and the shared-row kernels: one row, one short of and one past a 256-row block"""
    ops.refiner_out_case(f if h16_in else f32_of(f), Cp, M, alloc=Guarded())


@pytest.mark.parametrize("M", [1, 255, 257])
def test_refiner_apply_delta(f, M):
    """flow += (sx, sy) delta.xy, cert += delta.z with power-of-two scales: exact, as refiner_block_final_case asserts it"""
    lib, al = f.lib, Guarded()
    delta, flow, cert = al.inp(rnd(M, 4, seed=1)), al.inout(rnd(M, 2, seed=2)), al.inout(rnd(M, seed=3))
    f0, c0 = flow.clone(), cert.clone()
    ok(lib, lib.roma_op_refiner_apply_delta(P(delta), P(flow), P(cert), M, 0.25, 0.5, None))
    torch.cuda.synchronize()
    al.check()
    assert torch.equal(flow[:, 0], f0[:, 0] + 0.25 * delta[:, 0]) and torch.equal(flow[:, 1], f0[:, 1] + 0.5 * delta[:, 1])
    assert torch.equal(cert, c0 + delta[:, 2])


# Cc, E, K, ldf, ldd, h, w: the stride-1 case of test_refiner_input_grid_sample_warp (its smallest: the pix<9,6> kernel), its
# stride-2 case (the vector kernel) and a row of 2 C + E + Kcorr + 8 (a 24-column correlation slice and an 8-column tail)
REFINER_INPUT_CASES = [(9, 6, 0, 16, 24, 50, 47), (64, 16, 0, 64, 144, 33, 40), (64, 16, 24, 64, 64 + 64 + 16 + 24 + 8, 5, 9)]


@pytest.mark.parametrize("h16_in", [False, True])
@pytest.mark.parametrize("Cc,E,K,ldf,ldd,h,w", REFINER_INPUT_CASES)
def test_refiner_input(f, h16_in, Cc, E, K, ldf, ldd, h, w):
    """the case asserts the fate of the row: x and the sample, the embedding, the Kcorr columns untouched (its sentinel), zeros up
    to ldd.  With ROMA_RI_VEC=0 in the environment (test_refiner_input_wave_per_pixel_kernel) the C = 64 cases run
    refiner_input_kernel instead of the vector kernel; the launcher reports both under one name."""
    ff = f if h16_in else f32_of(f)
    with kernels_of(f.lib) as ran:
        d = ops.refiner_input_case(ff, Cc, E, K, ldf, ldd, h, w, alloc=Guarded())
    assert ran == ["refiner_input_warp<C=%d,%s>" % (Cc, dtn(f, ff.dt))], ran
    assert finite(d)
    assert_columns(d, 2 * Cc + E + K, ldd, "zero", "d")


def test_refiner_input_wave_per_pixel_kernel():
    """the same cases, bounds and guards in a child whose environment switches the vector kernel off (the switch is read once
    per process): 3 cases x 2 types x 2 libraries"""
    out = run_child([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "gpu",
                     os.path.join("tests", "test_gpu_extents.py") + "::test_refiner_input"], {"ROMA_RI_VEC": "0"})
    assert "12 passed" in out and "skipped" not in out and "failed" not in out, out[-3000:]


# ================================================================================================ local correlation
LC_PATHS = [(0, 1), (1, 1), (1, 0), (2, 0)]  # (lc_mode, lc_bin): tiles + sorted work list, every tile on the list, per-query gathers, per pixel


def lc_inputs(h16_tdt, c, h, w):
    from oracle import roma_oracle
    B = 2
    f0, f1 = rnd(B, c, h, w, seed=1), rnd(B, c, h, w, seed=2)
    warp = roma_oracle.pixel_grid(B, h, w) * 1.15 + 0.08 + rnd(B, 2, h, w, seed=3, std=0.004)
    if h > 2:
        warp[:, :, h // 2] += rnd(B, 2, w, seed=4, std=0.5)   # an incoherent row
        warp[1, :, :2, :2] = 3.0                               # far outside: all taps zero
    if h16_tdt is not None:
        f0, f1 = f0.to(h16_tdt), f1.to(h16_tdt)
    return f0, f1, warp.contiguous()


def lc_close(f, dt, got, ref):
    """test_local_corr_tiled_gather_and_legacy_paths_agree (f32, bf16), test_local_corr_window_f16"""
    atol, rtol = (1e-4, 1e-5) if dt == F32 else ((1e-3, 1e-4) if f.dt == BF16 else (2e-4, 1e-4))
    assert torch.allclose(got, ref, atol=atol, rtol=rtol), float((got - ref).abs().max())


@pytest.mark.parametrize("h,w", [(1, 1), (5, 9)])
@pytest.mark.parametrize("r", [2, 3, 7])
def test_local_corr_window(f, r, h, w):
    """The radii of the model (REF_RAD in arch.h: 7, 3, 2; scales with radius 0 launch nothing), the smallest channel count the
    tiled form takes (one 128-byte chunk: 64 16-bit, 32 f32 channels), every path, ldo = K + 8: the eight columns behind each
    row are untouched.  16-bit output (what the model writes into the refiner's d) has no parity bound of its own: extents and
    the bits of the f32 output rounded once."""
    from oracle import roma_oracle
    lib, B, K = f.lib, 2, (2 * r + 1) ** 2
    ldo = K + 8
    for dt in (f.dt, F32):
        c = 32 if dt == F32 else 64
        f0, f1, warp = lc_inputs(None if dt == F32 else f.tdt, c, h, w)
        ref = roma_oracle.local_correlation(f0.float(), f1.float(), r, warp)
        f0n, f1n = f0.permute(0, 2, 3, 1).contiguous(), f1.permute(0, 2, 3, 1).contiguous()
        wn = warp.permute(0, 2, 3, 1).contiguous()
        for mode, binned in LC_PATHS:
            al = Guarded()
            out = al.out((B, h * w, ldo), torch.float32)
            with tuned(lib, lc_mode=mode, lc_bin=binned), kernels_of(lib) as ran:
                ok(lib, lib.roma_op_local_corr_window(P(al.inp(f0n)), P(al.inp(f1n)), P(al.inp(wn)), P(out), B, h, w, c, r, c ** -0.5, ldo,
                                                      dt, F32, None))
            assert ran == ["local_corr_window_kernel<%d,%s>" % (r, dtn(f, dt))], ran
            al.check()
            assert_columns(out, K, ldo, "untouched", "out (lc_mode %d, lc_bin %d)" % (mode, binned))
            got = out[:, :, :K].cpu().permute(0, 2, 1).reshape(B, K, h, w)
            lc_close(f, dt, got, ref)
            if dt != F32:
                al16 = Guarded()
                out16 = al16.out((B, h * w, ldo), f.tdt)
                with tuned(lib, lc_mode=mode, lc_bin=binned):
                    ok(lib, lib.roma_op_local_corr_window(P(al16.inp(f0n)), P(al16.inp(f1n)), P(al16.inp(wn)), P(out16), B, h, w, c, r,
                                                          c ** -0.5, ldo, dt, dt, None))
                    torch.cuda.synchronize()
                al16.check()
                assert_columns(out16, K, ldo, "untouched", "16-bit out (lc_mode %d, lc_bin %d)" % (mode, binned))
                assert finite(out16[:, :, :K])


@pytest.mark.parametrize("h,w", [(1, 1), (5, 9)])
@pytest.mark.parametrize("r", [2, 3, 7])
def test_local_corr_window_caller_scratch(f, r, h, w):
    """roma_op_local_corr_window_ws inside exactly roma_op_local_corr_window_workspace(...) bytes of guarded scratch, on the
    default path and with every tile on the sorted work list"""
    from oracle import roma_oracle
    lib, B, K, c = f.lib, 2, (2 * r + 1) ** 2, 64
    f0, f1, warp = lc_inputs(f.tdt, c, h, w)
    ref = roma_oracle.local_correlation(f0.float(), f1.float(), r, warp)
    f0n, f1n = f0.permute(0, 2, 3, 1).contiguous(), f1.permute(0, 2, 3, 1).contiguous()
    wn = warp.permute(0, 2, 3, 1).contiguous()
    nbytes = lib.roma_op_local_corr_window_workspace(B, h, w, r)
    assert nbytes > 0 and nbytes % 4 == 0
    for mode in (0, 1):
        al = Guarded()
        ws = al.out((nbytes // 4,), torch.int32)
        out = al.out((B, h * w, K + 8), torch.float32)
        with tuned(lib, lc_mode=mode, lc_bin=1):
            ok(lib, lib.roma_op_local_corr_window_ws(P(al.inp(f0n)), P(al.inp(f1n)), P(al.inp(wn)), P(out), B, h, w, c, r, c ** -0.5, K + 8,
                                                     f.dt, F32, P(ws), nbytes, None))
            torch.cuda.synchronize()
        al.check()
        assert_columns(out, K, K + 8, "untouched", "out")
        lc_close(f, f.dt, out[:, :, :K].cpu().permute(0, 2, 1).reshape(B, K, h, w), ref)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 9)])
@pytest.mark.parametrize("r", [2, 7])
def test_local_corr_general(f, r, h, w):
    """roma_op_local_corr (per-tap coordinates, out [B, HW, K] dense) on f32 features; bound of test_local_corr_reference_golden"""
    from oracle import roma_oracle
    lib, B, K, c = f.lib, 2, (2 * r + 1) ** 2, 32
    f0, f1, warp = lc_inputs(None, c, h, w)
    ref = roma_oracle.local_correlation(f0, f1, r, warp)
    lw = torch.meshgrid(torch.linspace(-2 * r / h, 2 * r / h, 2 * r + 1), torch.linspace(-2 * r / w, 2 * r / w, 2 * r + 1), indexing="ij")
    lw = torch.stack((lw[1], lw[0]), dim=-1).reshape(1, K, 2)
    coords = (warp.permute(0, 2, 3, 1)[..., None, :] + lw[:, None, None]).reshape(B, h * w, K, 2).contiguous()
    al = Guarded()
    out = al.out((B, h * w, K), torch.float32)
    f0s = (f0.reshape(B, c, h * w).permute(0, 2, 1) / (c ** 0.5)).contiguous()
    ok(lib, lib.roma_op_local_corr(P(al.inp(f0s)), P(al.inp(f1.permute(0, 2, 3, 1).contiguous())), P(al.inp(coords)), P(out), B, h, w, c, K, 0,
                                   F32, F32, None))
    torch.cuda.synchronize()
    al.check()
    got = out.cpu().permute(0, 2, 1).reshape(B, K, h, w)
    assert torch.allclose(got, ref, atol=5e-5, rtol=1e-5), float((got - ref).abs().max())


# ================================================================================================ layernorm, attention
@pytest.mark.parametrize("in16", [False, True])
@pytest.mark.parametrize("D", [512, 1024, 2048])
@pytest.mark.parametrize("M", [1, 3])
def test_layernorm(f, M, D, in16):
    ops.layernorm_case(f, M, in16, alloc=Guarded(), D=D)


@pytest.mark.parametrize("B,heads,hd,N", [(1, 1, 64, 1), (2, 2, 64, 127), (1, 2, 64, 128), (1, 2, 64, 129), (1, 1, 128, 130)])
@pytest.mark.parametrize("h16_in", [False, True])
def test_qkv_scatter_and_attention(f, h16_in, B, heads, hd, N):
    """q, k, V^T guarded and zero-initialised: the rows [N, npad) are still zero afterwards (roma_hip.h: "the padding rows must
    stay zero"), `out` is guarded"""
    ff = f if h16_in else f32_of(f)
    with kernels_of(f.lib) as ran:
        q, k, vt, out = ops._attention_case(ff, B, heads, hd, N, alloc=Guarded())
    assert "attn_%s_kernel<%d>" % (dtn(f, ff.dt), hd) in ran, ran
    tail = (q.shape[2] - N) * hd
    assert_columns(q[:, :, N:].reshape(B * heads, tail), 0, tail, "zero", "q rows [N, npad)")
    assert_columns(k[:, :, N:].reshape(B * heads, tail), 0, tail, "zero", "k rows [N, npad)")
    assert_columns(vt, N, vt.shape[3], "zero", "V^T columns [N, npad)")
    assert finite(out)


# ================================================================================================ elementwise
@pytest.mark.parametrize("B,H,W,Cc", [(1, 2, 2, 4), (2, 5, 7, 12)])
@pytest.mark.parametrize("h16_in", [False, True])
def test_maxpool2x2(f, h16_in, B, H, W, Cc):
    ff = f if h16_in else f32_of(f)
    x = rnd(B, H, W, Cc, seed=1).to(ff.tdt)
    al = Guarded()
    out = al.out((B, H // 2, W // 2, Cc), ff.tdt)
    ok(f.lib, f.lib.roma_op_maxpool2x2(P(al.inp(x)), P(out), B, H, W, Cc, ff.dt, None))
    torch.cuda.synchronize()
    al.check()
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(out.cpu().float(), ref)  # a maximum is one of its operands


@pytest.mark.parametrize("B,hin,win,hout,wout,nc", [(1, 1, 1, 1, 1, 1), (2, 5, 7, 9, 3, 3)])
def test_resize_bilinear(f, B, hin, win, hout, wout, nc):
    x = rnd(B, nc, hin, win, seed=1)
    al = Guarded()
    out = al.out((B, hout, wout, nc), torch.float32)
    ok(f.lib, f.lib.roma_op_resize_bilinear(P(al.inp(x.permute(0, 2, 3, 1).contiguous())), P(out), B, hin, win, hout, wout, nc, None))
    torch.cuda.synchronize()
    al.check()
    ref = F.interpolate(x, size=(hout, wout), mode="bilinear", align_corners=False)
    assert torch.allclose(out.cpu().permute(0, 3, 1, 2), ref, atol=2e-5), float((out.cpu().permute(0, 3, 1, 2) - ref).abs().max())


@pytest.mark.parametrize("M", [1, 3])
def test_cls_to_flow(f, M):
    """the first M pixels of the reference's golden (test_cls_to_flow_reference_golden); ld = 4104: eight columns behind the gate"""
    g = np.load(os.path.join(GOLDEN, "ops_reference.npz"))
    cls = torch.from_numpy(g["c2f_cls"])
    assert cls.shape[0] * cls.shape[2] * cls.shape[3] >= M
    logits = torch.zeros((M, 4104))
    logits[:, :4096] = cls.permute(0, 2, 3, 1).reshape(-1, 4096)[:M]
    logits[:, 4096] = 7.0
    al = Guarded()
    flow, cert = al.out((M, 2), torch.float32), al.out((M,), torch.float32)
    ok(f.lib, f.lib.roma_op_cls_to_flow(P(al.inp(logits)), 4104, P(flow), P(cert), M, None))
    torch.cuda.synchronize()
    al.check()
    assert torch.allclose(flow.cpu(), torch.from_numpy(g["c2f_flow"]).reshape(-1, 2)[:M], atol=1e-5)
    assert torch.all(cert.cpu() == 7.0)


@pytest.mark.parametrize("n", [4, 1028])
def test_convert_from_bf16(f, n):
    """bfloat16 bits to the library's own 16-bit format: x.float().half() bit for bit in the binary16 library (the values of
    test_convert_from_bf16_is_torch_half, overflow and gradual underflow included), the same bits in the bfloat16 library"""
    x = (torch.randn(n, generator=torch.Generator().manual_seed(3)) * torch.exp2((torch.arange(n) % 49 - 30).float())).bfloat16()
    al = Guarded()
    out = al.out((n,), f.tdt)
    ok(f.lib, f.lib.roma_op_convert_from_bf16(P(al.inp(x)), P(out), n, None))
    torch.cuda.synchronize()
    al.check()
    assert torch.equal(out.cpu().view(torch.int16), x.float().to(f.tdt).view(torch.int16))


# ================================================================================================ Tiny RoMa operators
def tdev(al, a):
    return al.inp(torch.from_numpy(np.ascontiguousarray(a)))


def tiny_ratio(name, got, ref, bound):
    r = tc.ratio(got.cpu().numpy(), ref, bound)
    print(f"{name}: max(err / bound) = {r:.4f}")
    assert r <= 1, (name, r)


def test_tiny_conv2d_nhwc(f):
    """the smallest accepted case of each operator from tests/tiny_ops_cases.py, against its float64 reference and derived bound;
    here the inputs are guarded as well (tests/test_gpu_tiny_ops.py guards the outputs)"""
    lib = f.lib
    for case in (tc.CONV_CASES[1], tc.CONV_CASES[0]):  # the 1x1 form and a padded 3x3 with Cin = 1
        B, H, W, Cin, Cout, K, S, Pd = case
        x, w, bias, res = tc.conv_inputs(case)
        Ho, Wo = tc.conv_out_size(H, W, K, S, Pd)
        ref, bound = tc.conv_ref(x, w, bias, res, K, S, Pd, 1)
        al = Guarded()
        out = al.out((B, Ho, Wo, Cout), torch.float32)
        ok(lib, lib.roma_op_conv2d_nhwc(P(tdev(al, x)), P(tdev(al, w)), P(tdev(al, bias)), P(tdev(al, res)), P(out), B, H, W, Cin, Cout, K, S, Pd,
                                        1, None))
        torch.cuda.synchronize()
        al.check()
        tiny_ratio(f"conv2d_nhwc {case}", out, ref, bound)


def test_tiny_avgpool_instnorm_nchw_add3(f):
    lib = f.lib
    case = tc.AVGPOOL_CASES[3]
    B, H, W, Cc, k = case
    x = tc.avgpool_inputs(case)
    ref, bound = tc.avgpool_ref(x, k)
    al = Guarded()
    out = al.out((B, H // k, W // k, Cc), torch.float32)
    ok(lib, lib.roma_op_avgpool_nhwc(P(tdev(al, x)), P(out), B, H, W, Cc, k, None))
    torch.cuda.synchronize()
    al.check()
    tiny_ratio(f"avgpool_nhwc {case}", out, ref, bound)

    for case in (tc.INSTNORM_CASES[3], tc.INSTNORM_CASES[0]):
        B, H, W, Cc, eps = case
        x = tc.instnorm_inputs(case)
        ref, bound = tc.instnorm_ref(x, eps)
        al = Guarded()
        out = al.out((B, H, W, 1), torch.float32)
        ok(lib, lib.roma_op_gray_instnorm(P(tdev(al, x)), P(out), B, H, W, Cc, eps, None))
        torch.cuda.synchronize()
        al.check()
        if H * W == 1:
            assert bool((out == 0).all())  # variance 0 (test_gray_instnorm_zero_variance)
        else:
            tiny_ratio(f"gray_instnorm {case}", out, ref, bound)

    case = tc.NCHW_CASES[0]
    B, Cc, H, W = case
    x = tc.normal(tc.gen(5, *case), B, Cc, H, W)
    al = Guarded()
    out = al.out((B, H, W, Cc), torch.float32)
    ok(lib, lib.roma_op_nchw_to_nhwc(P(tdev(al, x)), P(out), B, Cc, H, W, None))
    torch.cuda.synchronize()
    al.check()
    assert torch.equal(out.cpu(), torch.from_numpy(x).permute(0, 2, 3, 1).contiguous())

    for n in (1, 255):
        a, b, c = tc.add3_inputs(n)
        al = Guarded()
        out = al.out((n,), torch.float32)
        ok(lib, lib.roma_op_add3(P(tdev(al, a)), P(tdev(al, b)), P(tdev(al, c)), P(out), n, None))
        torch.cuda.synchronize()
        al.check()
        assert torch.equal(out.cpu(), (torch.from_numpy(a) + torch.from_numpy(b)) + torch.from_numpy(c))


def test_tiny_matcher_ops(f):
    lib = f.lib
    case = tc.POS_CASES[0]
    B, H1, W1, H0, W0, _ = case
    cv = tc.pos_inputs(case)
    for exact in (0, 1):
        ref, bound = tc.pos_embed_ref(cv, H1, W1, exact)
        al = Guarded()
        out = al.out((B, H0 * W0, 2), torch.float32)
        ok(lib, lib.roma_op_tiny_pos_embed(P(tdev(al, cv)), P(out), B, H1, W1, H0, W0, exact, None))
        torch.cuda.synchronize()
        al.check()
        tiny_ratio(f"tiny_pos_embed {case} exact_softmax={exact}", out, ref, bound)

    case = tc.MATCHER_CASES[2]
    B, H, W, H1, W1, Cc, Cp, wc = case
    f0, f1, warp = tc.matcher_inputs(case)
    ref, bound = tc.matcher_sample_ref(f1, warp)
    al = Guarded()
    out = al.out((B, H, W, Cp), torch.float32)
    ok(lib, lib.roma_op_tiny_matcher_input(P(tdev(al, f0)), P(tdev(al, f1)), P(tdev(al, warp)), wc, P(out), B, H, W, H1, W1, Cc, Cp, None))
    torch.cuda.synchronize()
    al.check()
    got = out.cpu().numpy()
    assert np.array_equal(tc.bits(got[..., :Cc]), tc.bits(f0)) and np.array_equal(tc.bits(got[..., 2 * Cc:2 * Cc + 2]), tc.bits(warp[..., :2]))
    assert_columns(out, 2 * Cc + 2, Cp, "zero", "d")
    assert not np.isnan(got[..., Cc:2 * Cc]).any()
    tiny_ratio(f"tiny_matcher_input {case}", out[..., Cc:2 * Cc], ref, bound)

    for case in (tc.UPDATE_CASES[0], tc.UPDATE_CASES[-2]):  # (2, 3, 1) and (3, 4, 255): the fourth delta column is NaN
        nb, ldd, npix = case
        base, delta = tc.update_inputs(case)
        ref, bound = tc.update_ref(base, delta)
        al = Guarded()
        out = al.out((npix, 3), torch.float32)
        ok(lib, lib.roma_op_tiny_update(P(tdev(al, base)), nb, P(tdev(al, delta)), ldd, tc.UPDATE_SCALE[0], tc.UPDATE_SCALE[1], P(out), npix, None))
        torch.cuda.synchronize()
        al.check()
        tiny_ratio(f"tiny_update {case}", out, ref, bound)

    for case in (tc.FINAL_CASES[1], tc.FINAL_CASES[0]):
        m = tc.final_inputs(case)
        B, H, W, _ = m.shape
        ref, _ = tc.final_ref(m)
        al = Guarded()
        warp, cert = al.out((B, H, W, 4), torch.float32), al.out((B, H, W), torch.float32)
        ok(lib, lib.roma_op_tiny_final(P(tdev(al, m)), P(warp), P(cert), B, H, W, None))
        torch.cuda.synchronize()
        al.check()
        wn = warp.cpu().numpy()
        assert np.array_equal(tc.bits(wn[..., 2:]), tc.bits(m[..., :2]))
        tiny_ratio(f"tiny_final grid {case}", warp[..., :2], ref[..., :2], tc.FINAL_GRID_BOUND)
        r = tc.check_final_cert(cert.cpu().numpy(), m)
        assert r <= 1, r


# ================================================================================================ GP, Cholesky
@pytest.mark.parametrize("b,h,w", [(1, 2, 3), (2, 8, 8)])
@pytest.mark.parametrize("h16_in", [False, True])
def test_gp(f, h16_in, b, h, w):
    """n = 6 (padded to one 64-block with the identity) and n = 64; mu guarded, the features guarded"""
    ops.gp_case(f if h16_in else f32_of(f), b, h, w, alloc=Guarded())


@pytest.mark.parametrize("aug", [False, True])
@pytest.mark.parametrize("n,d", [(64, 8), (128, 8), (128, 64)])
def test_cholesky_solve_t(f, n, d, aug):
    """batch 2 in the separate and in the augmented storage form (one (n + d) x n matrix per item); d = 8 runs the right-looking
    chain, d = 64 augmented the block-column kernel (it asks for d % 64 == 0).  A / F^T, L^T and both tables of block inverses
    are guarded (L^T is a workspace: the block-column form leaves part of it unwritten, so only its guards are looked at).
    Reference and bounds: test_cholesky_solve."""
    lib, batch = f.lib, 2
    y = rnd(batch, n, 32, seed=1)
    yn = y / y.norm(dim=-1, keepdim=True)
    A = torch.exp((yn @ yn.transpose(1, 2) - 1.0) / 0.2) + 0.1 * torch.eye(n)
    Fm = rnd(batch, n, d, seed=2)
    Lref = torch.linalg.cholesky(A.double())
    ref = torch.cholesky_solve(Fm.double(), Lref)
    al = Guarded()
    if aug:
        buf = al.out((batch, n + d, n), torch.float32)
        buf[:, :n] = A.cuda()
        buf[:, n:] = Fm.transpose(1, 2).cuda()
        Ap, Fp = P(buf), C.c_void_p(buf.data_ptr() + n * n * 4)
        Aview, Fview = buf[:, :n], buf[:, n:]
    else:
        Aview, Fview = al.inout(A), al.inout(Fm.transpose(1, 2).contiguous())
        Ap, Fp = P(Aview), P(Fview)
    LT = al.out((batch, n, n), torch.float32)
    Linv, LinvT = al.out((batch, n // 64, 64, 64), torch.float32), al.out((batch, n // 64, 64, 64), torch.float32)
    ok(lib, lib.roma_op_cholesky_solve_t(Ap, Fp, P(LT), P(Linv), P(LinvT), n, d, batch, None))
    torch.cuda.synchronize()
    al.check()
    X = Fview.cpu().transpose(1, 2).double()
    assert torch.allclose(X, ref, atol=2e-4, rtol=1e-4), float((X - ref).abs().max())
    assert torch.allclose(torch.tril(Aview.cpu().double()), Lref, atol=1e-4)
    assert finite(Linv) and finite(LinvT)
    assert torch.equal(Linv.transpose(2, 3), LinvT)  # test_cholesky_solve_augmented_storage_forms_agree
