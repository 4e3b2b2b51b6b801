"""Every Tiny RoMa operator of csrc/tiny.hip, plus roma_op_resize_bilinear and the correlation GEMM as TinyRoMa calls them, on
the device through the C ABI (ctypes) against the float64 references of tests/tiny_ops_cases.py, each output element held to
the derived bound of its operator (test_cpu_tiny_ops.py shows that a plain f32 evaluation stays within half of it).  Every
test prints max(err / bound) and asserts it <= 1; the output-writing operators write into a buffer with poisoned guard rows in
front of the output and behind it.  tests/test_gpu_tiny.py stays the end-to-end check against the reference's goldens.

Worst max(err / bound) per operator on an MI355X:
  conv2d_nhwc 0.357 (the 1x1 skip1 form; 0.082 on the misaligned input)   avgpool_nhwc 0.129   gray_instnorm 0.027
  tiny_pos_embed 0.039 (either softmax)   tiny_matcher_input 0.242   tiny_update 0.499 (one rounding of two under 2U)
  tiny_final 0.242 grid, 0.142 certainty   resize_bilinear 0.129   correlation GEMM 0.091   compiled stacks 0.192
  nchw_to_nhwc, add3, the copied channels, the identity resize: bit-exact.
Two things the kernels got wrong when these tests first ran, both fixed in tiny.hip: gray_instnorm gave 6.2e-6 for a
single pixel (the gray value's product fused into the subtraction of its own rounded mean), and tiny_final gave certainty 0
at logit -90, where e^90 overflows f32 and sigmoid is 8.2e-40.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tiny_ops_cases as tc
from test_gpu_views import _guarded, _guards_intact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = 0
POISON = -7.0


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available()
    return built_lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_KEEP = []


def P(t):
    """device pointer; the tensor lives until the call has run (an inline `dev(x)` would otherwise hand its memory to the next one)"""
    if t is None:
        return None
    _KEEP.append(t)
    return C.c_void_p(t.data_ptr())


def call(lib, fn, *args):
    """the operator on the default stream, synchronised; 0 or the library's error text"""
    rc = fn(*args, None)
    torch.cuda.synchronize()
    _KEEP.clear()
    assert rc == 0, lib.roma_last_error().decode()


def refused(fn, *args):
    rc = fn(*args, None)
    torch.cuda.synchronize()
    _KEEP.clear()
    return rc != 0


def out_buf(*shape):
    return _guarded(shape, torch.float32, POISON)


def fetch(buf, v):
    """the output, once the guards in front of it and behind it are seen untouched"""
    assert _guards_intact(buf, v, POISON)
    return v.cpu().numpy()


def untouched(buf):
    return bool((buf == POISON).all())


def report(name, r):
    print(f"{name}: max(err / bound) = {r:.4f}")
    assert r <= 1, (name, r)


# ------------------------------------------------------------------------------------------------ conv2d_nhwc
def _conv(lib, x, w, bias, res, case, relu, misalign=False):
    B, H, W, Cin, Cout, K, S, P_ = case
    Ho, Wo = tc.conv_out_size(H, W, K, S, P_)
    if misalign:  # one float behind a 16-byte boundary: the scalar fallback
        xb = torch.empty(x.size + 1, device=DEV, dtype=torch.float32)
        xd = xb[1:].view(*x.shape)
        xd.copy_(dev(x))
        assert xd.data_ptr() % 16 == 4
    else:
        xd = dev(x)
        assert xd.data_ptr() % 16 == 0
    wd, bd, rd = dev(w), (dev(bias) if bias is not None else None), (dev(res) if res is not None else None)
    buf, out = out_buf(B, Ho, Wo, Cout)
    call(lib, lib.roma_op_conv2d_nhwc, P(xd), P(wd), P(bd), P(rd), P(out), B, H, W, Cin, Cout, K, S, P_, relu)
    return fetch(buf, out)


@pytest.mark.parametrize("case", tc.CONV_CASES, ids=str)
def test_conv2d_nhwc(lib, case):
    K, S, P_ = case[5:]
    x, w, bias, res = tc.conv_inputs(case)
    worst = 0.0
    for hb, relu, hr in tc.CONV_FLAGS:  # with and without bias, ReLU, residual; ReLU comes before the residual
        b_, r_ = (bias if hb else None), (res if hr else None)
        ref, bound = tc.conv_ref(x, w, b_, r_, K, S, P_, relu)
        r = tc.ratio(_conv(lib, x, w, b_, r_, case, relu), ref, bound)
        print(f"  bias={hb} relu={relu} res={hr}: {r:.4f}")
        worst = max(worst, r)
    report(f"conv2d_nhwc {case}", worst)


def test_conv2d_nhwc_misaligned_input(lib):
    case = tc.CONV_MISALIGNED
    K, S, P_ = case[5:]
    x, w, bias, res = tc.conv_inputs(case)
    assert case[3] % 4 == 0
    ref, bound = tc.conv_ref(x, w, bias, res, K, S, P_, 1)
    report(f"conv2d_nhwc {case}, in one float off a 16-byte boundary", tc.ratio(_conv(lib, x, w, bias, res, case, 1, misalign=True), ref, bound))


@pytest.mark.parametrize("case", tc.CONV_REFUSALS, ids=str)
def test_conv2d_nhwc_refuses(lib, case):
    B, H, W, Cin, Cout, K, S, P_ = case
    x = dev(tc.normal(tc.gen(1), B, H, W, Cin))
    w, b = dev(tc.normal(tc.gen(2), K * K * Cin, 8)), dev(tc.normal(tc.gen(3), 8))
    buf = torch.full((B * (H + 2) * (W + 2) * 8,), POISON, device=DEV, dtype=torch.float32)  # room for any reading of the output size
    assert refused(lib.roma_op_conv2d_nhwc, P(x), P(w), P(b), None, P(buf), B, H, W, Cin, Cout, K, S, P_, 0)
    assert lib.roma_last_error().decode().startswith("conv2d_nhwc") and untouched(buf)


# ------------------------------------------------------------------------------------------------ avgpool_nhwc
@pytest.mark.parametrize("case", tc.AVGPOOL_CASES, ids=str)
def test_avgpool_nhwc(lib, case):
    B, H, W, Cc, k = case
    x = tc.avgpool_inputs(case)
    ref, bound = tc.avgpool_ref(x, k)
    buf, out = out_buf(B, H // k, W // k, Cc)
    call(lib, lib.roma_op_avgpool_nhwc, P(dev(x)), P(out), B, H, W, Cc, k)
    report(f"avgpool_nhwc {case}", tc.ratio(fetch(buf, out), ref, bound))


def test_avgpool_nhwc_refuses(lib):
    B, H, W, Cc, k = tc.AVGPOOL_REFUSAL
    x = dev(tc.normal(tc.gen(4), B, H, W, Cc))
    buf = torch.full((B * H * W * Cc,), POISON, device=DEV, dtype=torch.float32)
    assert refused(lib.roma_op_avgpool_nhwc, P(x), P(buf), B, H, W, Cc, k) and untouched(buf)


# ------------------------------------------------------------------------------------------------ gray_instnorm
def _instnorm(lib, x, eps):
    B, H, W, Cc = x.shape
    buf, out = out_buf(B, H, W, 1)
    call(lib, lib.roma_op_gray_instnorm, P(dev(x)), P(out), B, H, W, Cc, eps)
    return fetch(buf, out)


@pytest.mark.parametrize("case", tc.INSTNORM_CASES, ids=str)
def test_gray_instnorm(lib, case):
    x = tc.instnorm_inputs(case)
    ref, bound = tc.instnorm_ref(x, case[4])
    report(f"gray_instnorm {case}", tc.ratio(_instnorm(lib, x, case[4]), ref, bound))


def test_gray_instnorm_zero_variance(lib):
    for x in (tc.instnorm_inputs(tc.INSTNORM_CASES[3]), tc.instnorm_constant()):
        got = _instnorm(lib, x, 1e-5)
        assert np.isfinite(got).all() and (got == 0).all(), got.ravel()[:8]
    report("gray_instnorm, variance 0", 0.0)


# ------------------------------------------------------------------------------------------------ nchw_to_nhwc, add3
@pytest.mark.parametrize("case", tc.NCHW_CASES, ids=str)
def test_nchw_to_nhwc_is_permute(lib, case):
    B, Cc, H, W = case
    x = tc.normal(tc.gen(5, *case), B, Cc, H, W)
    buf, out = out_buf(B, H, W, Cc)
    call(lib, lib.roma_op_nchw_to_nhwc, P(dev(x)), P(out), B, Cc, H, W)
    want = torch.from_numpy(x).permute(0, 2, 3, 1).contiguous().numpy()
    report(f"nchw_to_nhwc {case}", 0.0 if np.array_equal(tc.bits(fetch(buf, out)), tc.bits(want)) else np.inf)


@pytest.mark.parametrize("n", tc.ADD3_SIZES)
def test_add3_is_left_to_right(lib, n):
    a, b, c = tc.add3_inputs(n)
    ta, tb, tcc = (torch.from_numpy(v) for v in (a, b, c))
    for third, want in ((c, (ta + tb) + tcc), (None, ta + tb)):
        buf, out = out_buf(n)
        call(lib, lib.roma_op_add3, P(dev(a)), P(dev(b)), P(dev(third)) if third is not None else None, P(out), n)
        assert np.array_equal(tc.bits(fetch(buf, out)), tc.bits(want.numpy())), (n, third is None)
    report(f"add3 n={n}", 0.0)


# ------------------------------------------------------------------------------------------------ tiny_pos_embed
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("case", tc.POS_CASES, ids=str)
def test_tiny_pos_embed(lib, case, exact):
    B, H1, W1, H0, W0, kind = case
    cv = tc.pos_inputs(case)  # with tied maxima in the first three queries: the first index wins
    ref, bound = tc.pos_embed_ref(cv, H1, W1, exact)
    buf, out = out_buf(B, H0 * W0, 2)
    call(lib, lib.roma_op_tiny_pos_embed, P(dev(cv)), P(out), B, H1, W1, H0, W0, exact)
    got = fetch(buf, out)
    ties = tc.ratio(got[:, :3], ref[:, :3], bound[:, :3])
    print(f"  the three queries with tied maxima: {ties:.4f}")
    report(f"tiny_pos_embed {case} exact_softmax={exact}", tc.ratio(got, ref, bound))


def test_tiny_pos_embed_refuses(lib):
    B, H1, W1, H0, W0 = tc.POS_REFUSAL
    cv = dev(tc.normal(tc.gen(6), B, H1 * W1, H0 * W0))
    buf = torch.full((B * H0 * W0 * 2,), POISON, device=DEV, dtype=torch.float32)
    assert refused(lib.roma_op_tiny_pos_embed, P(cv), P(buf), B, H1, W1, H0, W0, 0) and untouched(buf)


# ------------------------------------------------------------------------------------------------ tiny_matcher_input
@pytest.mark.parametrize("case", tc.MATCHER_CASES, ids=str)
def test_tiny_matcher_input(lib, case):
    B, H, W, H1, W1, Cc, Cp, wc = case
    f0, f1, warp = tc.matcher_inputs(case)
    ref, bound = tc.matcher_sample_ref(f1, warp)
    buf, out = out_buf(B, H, W, Cp)
    call(lib, lib.roma_op_tiny_matcher_input, P(dev(f0)), P(dev(f1)), P(dev(warp)), wc, P(out), B, H, W, H1, W1, Cc, Cp)
    got = fetch(buf, out)
    assert np.array_equal(tc.bits(got[..., :Cc]), tc.bits(f0))  # f0 and the warp bit for bit, the pad channels exactly 0
    assert np.array_equal(tc.bits(got[..., 2 * Cc:2 * Cc + 2]), tc.bits(warp[..., :2]))
    assert np.array_equal(tc.bits(got[..., 2 * Cc + 2:]), np.zeros((B, H, W, Cp - 2 * Cc - 2), dtype=np.int32))
    s = got[..., Cc:2 * Cc]
    xy = warp[..., :2].astype(np.float64)
    wild = ~np.isfinite(xy).all(axis=-1) | (np.abs(xy) > 1e6).any(axis=-1)
    assert not np.isnan(s).any() and (s[wild] == 0).all()  # +-1e30 and +-inf clamp: all-zero samples
    report(f"tiny_matcher_input {case}", tc.ratio(s, ref, bound))


def test_tiny_matcher_input_refuses(lib):
    B, H, W, H1, W1, Cc, Cp, wc = tc.MATCHER_REFUSAL
    f0, f1, warp = (dev(tc.normal(tc.gen(7, i), *s)) for i, s in enumerate(((B, H, W, Cc), (B, H1, W1, Cc), (B, H, W, wc))))
    buf = torch.full((B * H * W * (2 * Cc + 2),), POISON, device=DEV, dtype=torch.float32)
    assert refused(lib.roma_op_tiny_matcher_input, P(f0), P(f1), P(warp), wc, P(buf), B, H, W, H1, W1, Cc, Cp) and untouched(buf)


# ------------------------------------------------------------------------------------------------ tiny_update
@pytest.mark.parametrize("case", tc.UPDATE_CASES, ids=str)
def test_tiny_update(lib, case):
    nb, ldd, npix = case
    base, delta = tc.update_inputs(case)  # a fourth delta column is NaN
    ref, bound = tc.update_ref(base, delta)
    buf, out = out_buf(npix, 3)
    call(lib, lib.roma_op_tiny_update, P(dev(base)), nb, P(dev(delta)), ldd, tc.UPDATE_SCALE[0], tc.UPDATE_SCALE[1], P(out), npix)
    report(f"tiny_update {case}", tc.ratio(fetch(buf, out), ref, bound))


@pytest.mark.parametrize("case", tc.UPDATE_REFUSALS, ids=str)
def test_tiny_update_refuses(lib, case):
    nb, ldd, npix = case
    base, delta = dev(tc.normal(tc.gen(8), npix, nb)), dev(tc.normal(tc.gen(9), npix, max(ldd, 3)))
    buf = torch.full((npix * 3,), POISON, device=DEV, dtype=torch.float32)
    assert refused(lib.roma_op_tiny_update, P(base), nb, P(delta), ldd, 0.1, 0.1, P(buf), npix) and untouched(buf)


# ------------------------------------------------------------------------------------------------ tiny_final
@pytest.mark.parametrize("m", [tc.final_inputs(c) for c in tc.FINAL_CASES] + [tc.final_special_logits()], ids=lambda m: str(m.shape[:3]))
def test_tiny_final(lib, m):
    B, H, W, _ = m.shape
    ref, _ = tc.final_ref(m)
    (wbuf, warp), (cbuf, cert) = out_buf(B, H, W, 4), out_buf(B, H, W)
    call(lib, lib.roma_op_tiny_final, P(dev(m)), P(warp), P(cert), B, H, W)
    w, c = fetch(wbuf, warp), fetch(cbuf, cert)
    assert np.array_equal(tc.bits(w[..., 2:]), tc.bits(m[..., :2]))  # the flow bit for bit
    report(f"tiny_final grid {m.shape[:3]}", tc.ratio(w[..., :2], ref[..., :2], tc.FINAL_GRID_BOUND))
    report(f"tiny_final certainty {m.shape[:3]}", tc.check_final_cert(c, m))


# ------------------------------------------------------------------------------------------------ resize_bilinear
@pytest.mark.parametrize("case", tc.RESIZE_CASES, ids=str)
def test_resize_bilinear_as_tiny_roma_uses_it(lib, case):
    B, Hin, Win, Hout, Wout, nc = case
    x = tc.resize_inputs(case)
    ref, bound = tc.resize_ref(x, Hout, Wout)
    buf, out = out_buf(B, Hout, Wout, nc)
    call(lib, lib.roma_op_resize_bilinear, P(dev(x)), P(out), B, Hin, Win, Hout, Wout, nc)
    got = fetch(buf, out)
    if case == tc.RESIZE_IDENTITY:
        assert np.array_equal(tc.bits(got), tc.bits(x))
    report(f"resize_bilinear {case}", tc.ratio(got, ref, bound))


# ------------------------------------------------------------------------------------------------ correlation volume
@pytest.mark.parametrize("case", tc.CORR_CASES, ids=str)
def test_corr_volume_gemm(lib, case):
    """roma_op_gemm as TinyRoMa._forward_from_nhwc calls it: A = the features of image B, W = those of image A"""
    B, n1, n0, Cc = case
    f1, f0 = tc.corr_inputs(case)
    ref, bound = tc.corr_ref(f1, f0)
    buf, cv = out_buf(B, n1, n0)
    call(lib, lib.roma_op_gemm, P(dev(f1)), Cc, P(dev(f0)), Cc, P(cv), n0, n1, n0, Cc, B, n1 * Cc, n0 * Cc, n1 * n0, None, None, None, 0, 0,
         tc.corr_alpha(Cc), F32, F32)
    got = fetch(buf, cv)
    assert got.shape == ref.shape == (B, n1, n0)
    report(f"corr volume {case}", tc.ratio(got, ref, bound))


# ------------------------------------------------------------------------------------------------ the stack compiler
def _device_op(lib):
    def run(o, x):
        B, H, W, Cc = x.shape
        if o["op"] == "avgpool":
            buf, out = out_buf(B, H // o["k"], W // o["k"], Cc)
            call(lib, lib.roma_op_avgpool_nhwc, P(dev(x)), P(out), B, H, W, Cc, o["k"])
        else:
            assert Cc == o["cin"]
            buf, out = out_buf(B, *tc.conv_out_size(H, W, o["k"], o["s"], o["p"]), o["cout"])
            call(lib, lib.roma_op_conv2d_nhwc, P(dev(x)), P(o["w"]), P(o["b"]), None, P(out), B, H, W, Cc, o["cout"], o["k"], o["s"], o["p"], o["relu"])
        return fetch(buf, out)
    return run


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_compiled_stack_on_the_device(lib, name):
    from roma_amd.tiny import _compile_stack
    m, shape = tc.stacks()[name]
    ops = _compile_stack(m, torch.device(DEV))
    report(f"compiled stack {name} {shape}", tc.check_stack(m, ops, tc.stack_input(shape, 0), _device_op(lib)))


def test_tiny_roma_refuses_ceil_mode_at_construction(lib):
    """a backbone whose pooling rounds the output size up is refused when TinyRoMa is built, not computed with the floor"""
    from roma_amd.tiny import TinyRoMa
    nn = torch.nn
    x = nn.Module()
    x.norm = nn.InstanceNorm2d(1)
    for name in ("block1", "block2", "block3", "block4", "block5", "block_fusion"):
        setattr(x, name, nn.Sequential(nn.Conv2d(1, 4, 1)))
    x.skip1 = nn.Sequential(nn.AvgPool2d(4, 4, ceil_mode=True), nn.Conv2d(1, 4, 1))
    with pytest.raises(NotImplementedError):
        TinyRoMa(xfeat=x, device=DEV)
    x.skip1 = nn.Sequential(nn.AvgPool2d(4, 4), nn.Conv2d(1, 4, 1))
    TinyRoMa(xfeat=x, device=DEV)
