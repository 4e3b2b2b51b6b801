"""The yardsticks of tests/test_gpu_tiny_ops.py, checked without a GPU (tests/tiny_ops_cases.py):
  - every float64 reference against torch's own operator in float64, to 1e-12;
  - every f32 restatement (numpy float32 in the kernel's order, no FMA) within HALF of its operator's bound on every case, so a
    correct f32 kernel has as much room again for its own order of evaluation (tiny_update's bound, 2U for two roundings,
    leaves that room only to the fused form; the unfused one is held to the whole bound);
  - _compile_stack (roma_amd/tiny.py) on small stacks: the compiled list, evaluated with the float64 references, against the
    torch module layer by layer, and the stacks it must refuse."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tiny_ops_cases as tc

TOL = 1e-12


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.allclose(a, b, rtol=TOL, atol=TOL))


def _nchw(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _half(name, r):
    print(f"{name}: f32 restatement at {r:.3f} of the bound")
    assert r <= 0.5, (name, r)


# ------------------------------------------------------------------------------------------------ conv2d_nhwc
@pytest.mark.parametrize("case", tc.CONV_CASES, ids=str)
def test_conv_reference_and_restatement(case):
    B, H, W, Cin, Cout, K, S, P = case
    x, w, bias, res = tc.conv_inputs(case)
    wt = torch.from_numpy(w.astype(np.float64).reshape(K, K, Cin, Cout)).permute(3, 2, 0, 1)  # [Cout, Cin, K, K]
    worst, negative = 0.0, 0
    for hb, relu, hr in tc.CONV_FLAGS:
        b_, r_ = (bias if hb else None), (res if hr else None)
        ref, bound = tc.conv_ref(x, w, b_, r_, K, S, P, relu)
        t = F.conv2d(_nchw(x), wt, torch.from_numpy(bias.astype(np.float64)) if hb else None, stride=S, padding=P)
        t = F.relu(t) if relu else t
        t = t + _nchw(res) if hr else t  # ReLU before the residual
        assert _close(ref, _nhwc(t)), (case, hb, relu, hr)
        assert (bound > 0).all()
        worst = max(worst, tc.ratio(tc.conv_f32(x, w, b_, r_, K, S, P, relu), ref, bound))
        if relu and hr:  # the order of ReLU and residual shows: the other order differs by far more than the bound somewhere
            other = np.maximum(tc.conv_ref(x, w, b_, None, K, S, P, 0)[0] + res, 0.0)
            negative = max(negative, tc.ratio(other, ref, bound))
    assert negative > 1e3, negative
    _half(f"conv {case}", worst)


def test_conv_bound_counts_only_the_taps_inside_the_image():
    """all-ones data: the bound is (n + 3) U n with n = (taps inside) x Cin - 4 taps in a corner of a padded 3x3, 9 inside"""
    x, w = np.ones((1, 5, 5, 2), dtype=np.float32), np.ones((9 * 2, 4), dtype=np.float32)
    ref, bound = tc.conv_ref(x, w, None, None, 3, 1, 1, 0)
    assert ref[0, 0, 0, 0] == 8 and ref[0, 2, 2, 0] == 18 and ref[0, 0, 2, 0] == 12
    assert bound[0, 0, 0, 0] == (8 + 3) * tc.U * 8 and bound[0, 2, 2, 0] == (18 + 3) * tc.U * 18


# ------------------------------------------------------------------------------------------------ avgpool_nhwc
@pytest.mark.parametrize("case", tc.AVGPOOL_CASES, ids=str)
def test_avgpool_reference_and_restatement(case):
    k = case[4]
    x = tc.avgpool_inputs(case)
    ref, bound = tc.avgpool_ref(x, k)
    assert _close(ref, _nhwc(F.avg_pool2d(_nchw(x), k, k)))
    _half(f"avgpool {case}", tc.ratio(tc.avgpool_f32(x, k), ref, bound))


# ------------------------------------------------------------------------------------------------ gray_instnorm
@pytest.mark.parametrize("case", tc.INSTNORM_CASES, ids=str)
def test_instnorm_reference_and_restatement(case):
    eps = case[4]
    x = tc.instnorm_inputs(case)
    ref, bound = tc.instnorm_ref(x, eps)
    norm = torch.nn.InstanceNorm2d(1, eps=float(np.float32(eps))).double()
    if x.shape[1] * x.shape[2] > 1:
        assert _close(ref, _nhwc(norm(_nchw(x).mean(1, keepdim=True))))
    else:  # torch refuses a single pixel; its normalised value is 0 by definition
        assert (ref == 0).all()
    _half(f"gray_instnorm {case}", tc.ratio(tc.instnorm_f32(x, eps), ref, bound))
    if x.shape[1] * x.shape[2] > 1:
        # the unbiased variance (a 1 / HW effect) and a neighbour's statistics are both far outside the bound
        hw = x.shape[1] * x.shape[2]
        assert tc.ratio(ref * math.sqrt((hw - 1) / hw), ref, bound) > 10
        if x.shape[0] > 1:
            g = x.astype(np.float64).mean(axis=3, keepdims=True)
            rolled = (g - np.roll(g.mean(axis=(1, 2), keepdims=True), 1, axis=0)) / np.sqrt(g.var(axis=(1, 2), keepdims=True) + eps)
            assert tc.ratio(rolled, ref, bound) > 1e3


def test_instnorm_zero_variance_is_exactly_zero():
    for x in (tc.instnorm_inputs(tc.INSTNORM_CASES[3]), tc.instnorm_constant()):
        ref, _ = tc.instnorm_ref(x, 1e-5)
        out = tc.instnorm_f32(x, 1e-5)
        assert (ref == 0).all() and (out == 0).all() and np.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ tiny_pos_embed
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("case", tc.POS_CASES, ids=str)
def test_pos_embed_reference_and_restatement(case, exact):
    B, H1, W1, H0, W0, kind = case
    cv = tc.pos_inputs(case)
    ref, bound = tc.pos_embed_ref(cv, H1, W1, exact)
    c = torch.from_numpy(cv).double()
    gx = torch.linspace(-1 + 1 / W1, 1 - 1 / W1, W1, dtype=torch.float64).repeat(H1)
    gy = torch.linspace(-1 + 1 / H1, 1 - 1 / H1, H1, dtype=torch.float64).repeat_interleave(W1)
    if exact:
        p = torch.softmax(c, dim=1)
        want = torch.stack([(p * gx[None, :, None]).sum(1), (p * gy[None, :, None]).sum(1)], dim=-1)
    else:
        best = torch.argmax(torch.from_numpy(cv), dim=1)  # on the f32 values
        sub = c.reshape(B, H1, W1, -1)[:, ::4, ::4].reshape(B, -1, H0 * W0)
        p = torch.softmax(torch.cat([sub, best[:, None, :].double()], dim=1), dim=1)
        lx = torch.linspace(-1 + 4 / W1, 1 - 4 / W1, W1 // 4, dtype=torch.float64).repeat(H1 // 4)
        ly = torch.linspace(-1 + 4 / H1, 1 - 4 / H1, H1 // 4, dtype=torch.float64).repeat_interleave(W1 // 4)
        want = torch.stack([(p[:, :-1] * lx[None, :, None]).sum(1) + p[:, -1] * gx[best], (p[:, :-1] * ly[None, :, None]).sum(1) + p[:, -1] * gy[best]], dim=-1)
        # the tie rule: the first of the tied positions
        for q, tie in enumerate(tc.pos_ties(case)):
            assert (best[:, q] == tie[0]).all() and (cv[:, list(tie), q] == cv[:, :, q].max(axis=1, keepdims=True)).all()
            last = cv.copy()
            last[:, tie[0], q] = -100.0  # what an arg-max that takes the last maximum would see
            assert tc.ratio(tc.pos_embed_ref(last, H1, W1, 0)[0][:, q], ref[:, q], bound[:, q]) > 1e3
        if kind == "swamped":  # the index logit swamps the column: the grid point of the arg-max
            grid = torch.stack([gx[best], gy[best]], dim=-1).numpy()
            assert (best.numpy() >= 3 * H1 * W1 // 4 - 30).all() and tc.ratio(grid, ref, bound) <= 1
        if kind == "soft":  # the soft part decides: far from the grid point of the arg-max on most queries
            grid = torch.stack([gx[best], gy[best]], dim=-1).numpy()
            assert (np.abs(grid - ref).max(axis=-1) > 1e-3).mean() > 0.25
    assert _close(ref, want.numpy())
    _half(f"pos_embed {case} exact={exact}", tc.ratio(tc.pos_embed_f32(cv, H1, W1, exact), ref, bound))


def test_expf_allowance():
    assert 1 <= tc.expf_ulp() <= 3, tc.expf_ulp()


# ------------------------------------------------------------------------------------------------ tiny_matcher_input
@pytest.mark.parametrize("case", tc.MATCHER_CASES, ids=str)
def test_matcher_input_reference_and_restatement(case):
    f0, f1, warp = tc.matcher_inputs(case)
    ref, bound = tc.matcher_sample_ref(f1, warp)
    xy = warp[..., :2].astype(np.float64)
    wild = ~np.isfinite(xy).all(axis=-1) | (np.abs(xy) > 1e6).any(axis=-1)
    assert (ref[wild] == 0).all() and np.isfinite(ref).all()  # +-1e30 and +-inf sample zeros, no NaN
    xy[wild] = 5.0  # far outside, which torch samples as zeros as well
    want = F.grid_sample(_nchw(f1), torch.from_numpy(xy), mode="bilinear", padding_mode="zeros", align_corners=False)
    assert _close(ref, _nhwc(want))
    got = tc.matcher_sample_f32(f1, warp)
    assert np.isfinite(got).all() and (got[wild] == 0).all()
    _half(f"matcher_input {case}", tc.ratio(got, ref, bound))


def test_matcher_warp_holds_every_special_sample():
    """the two larger cases hold all of them; half a pixel outside a border samples exactly zero weight inside"""
    for case in tc.MATCHER_CASES[:2]:
        B, H, W, H1, W1, C, Cp, wc = case
        _, f1, warp = tc.matcher_inputs(case)
        xy = warp[..., :2].reshape(-1, 2)
        for v in (np.inf, -np.inf, np.float32(1e30), np.float32(-1e30), np.float32(-1 - 1 / W1), np.float32(1 + 1 / W1), np.float32(-1 - 1 / H1), np.float32(1 + 1 / H1)):
            assert (xy == v).any(), v
        assert ((xy == -1).all(axis=1)).any() and ((xy == 1).all(axis=1)).any()
        assert (np.abs(xy) > 1).any() and (np.abs(xy) < 1).all(axis=1).any()


# ------------------------------------------------------------------------------------------------ tiny_update, tiny_final
@pytest.mark.parametrize("case", tc.UPDATE_CASES, ids=str)
def test_update_reference_and_restatement(case):
    base, delta = tc.update_inputs(case)
    ref, bound = tc.update_ref(base, delta)
    assert np.isfinite(ref).all()  # the NaN column is not read
    b = torch.zeros(case[2], 3, dtype=torch.float64)
    b[:, :case[0]] = torch.from_numpy(base).double()
    s = torch.tensor([float(np.float32(tc.UPDATE_SCALE[0])), float(np.float32(tc.UPDATE_SCALE[1])), 1.0], dtype=torch.float64)
    assert _close(ref, (b + torch.from_numpy(delta[:, :3]).double() * s).numpy())
    _half(f"tiny_update {case}", tc.ratio(tc.update_f32(base, delta), ref, bound))
    assert tc.ratio(tc.update_f32(base, delta, fused=False), ref, bound) <= 1  # two roundings: past half, within the bound


@pytest.mark.parametrize("m", [tc.final_inputs(c) for c in tc.FINAL_CASES] + [tc.final_special_logits()], ids=lambda m: str(m.shape))
def test_final_reference_and_restatement(m):
    B, H, W, _ = m.shape
    warp, cert = tc.final_ref(m)
    assert _close(cert, torch.sigmoid(torch.from_numpy(m[..., 2]).double()).numpy())
    assert _close(warp[0, 0, :, 0], torch.linspace(-1 + 1 / W, 1 - 1 / W, W, dtype=torch.float64).numpy())
    assert _close(warp[0, :, 0, 1], torch.linspace(-1 + 1 / H, 1 - 1 / H, H, dtype=torch.float64).numpy())
    w32, c32 = tc.final_f32(m)
    assert np.array_equal(tc.bits(w32[..., 2:]), tc.bits(m[..., :2]))
    _half(f"tiny_final grid {m.shape}", tc.ratio(w32[..., :2], warp[..., :2], tc.FINAL_GRID_BOUND))
    _half(f"tiny_final certainty {m.shape}", tc.check_final_cert(c32, m))


def test_final_certainty_edges():
    """what the edge rule asks: sigmoid(20) rounds to 1 in f32, sigmoid(-20) and sigmoid(-90) do not round to 0, +-inf give 1 and 0"""
    m = tc.final_special_logits()
    _, cert = tc.final_ref(m)
    with np.errstate(under="ignore"):
        c = dict(zip(tc.FINAL_LOGITS, cert[0, 0].astype(np.float32).tolist()))
    assert c[0.0] == 0.5 and c[20.0] == 1.0 and c[90.0] == 1.0 and c[math.inf] == 1.0 and c[-math.inf] == 0.0
    assert 0 < c[-20.0] < 1e-8 and 0 < c[-90.0] < 1e-38
    zero = np.zeros_like(cert, dtype=np.float32)  # a kernel whose e^90 overflows returns 0 at -90: refused
    zero[0, 0, :4] = [0.5, 1.0, c[-20.0], 1.0]
    with pytest.raises(AssertionError):
        tc.check_final_cert(zero, m)


# ------------------------------------------------------------------------------------------------ resize_bilinear
@pytest.mark.parametrize("case", tc.RESIZE_CASES, ids=str)
def test_resize_reference_and_restatement(case):
    B, Hin, Win, Hout, Wout, nc = case
    x = tc.resize_inputs(case)
    ref, bound = tc.resize_ref(x, Hout, Wout)
    assert _close(ref, _nhwc(F.interpolate(_nchw(x), size=(Hout, Wout), mode="bilinear", align_corners=False)))
    got = tc.resize_f32(x, Hout, Wout)
    _half(f"resize_bilinear {case}", tc.ratio(got, ref, bound))
    if case == tc.RESIZE_IDENTITY:
        assert np.array_equal(tc.bits(got), tc.bits(x))
    elif Hin * Wout != Win * Hout:  # the two scales swapped: far outside the bound
        assert tc.ratio(tc.resize_ref(x, Hout, Wout, swap_scales=True)[0], ref, bound) > 1e3


# ------------------------------------------------------------------------------------------------ correlation volume
@pytest.mark.parametrize("case", tc.CORR_CASES, ids=str)
def test_corr_reference_and_restatement(case):
    B, n1, n0, C = case
    f1, f0 = tc.corr_inputs(case)
    ref, bound = tc.corr_ref(f1, f0)
    assert ref.shape == (B, n1, n0)
    want = torch.bmm(torch.from_numpy(f1).double(), torch.from_numpy(f0).double().transpose(1, 2)) * tc.corr_alpha(C)
    assert _close(ref, want.numpy())
    _half(f"corr volume {case}", tc.ratio(tc.corr_f32(f1, f0), ref, bound))


# ------------------------------------------------------------------------------------------------ nchw_to_nhwc, add3
def test_exact_operators_have_exact_references():
    a, b, c = tc.add3_inputs(257)
    assert np.array_equal(tc.bits((a + b) + c), tc.bits(((torch.from_numpy(a) + torch.from_numpy(b)) + torch.from_numpy(c)).numpy()))
    assert not np.array_equal(tc.bits((a + b) + c), tc.bits(a + (b + c)))  # the order of the additions shows in the bits


# ------------------------------------------------------------------------------------------------ the stack compiler
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_compile_stack_against_the_torch_module(name):
    from roma_amd.tiny import _compile_stack
    m, shape = tc.stacks()[name]
    ops = _compile_stack(m, "cpu")
    assert [o["op"] for o in ops] == {"a": ["conv"] * 3, "b": ["avgpool", "conv"], "c": ["conv"] * 2}[name]
    assert [o.get("relu") for o in ops] == {"a": [1, 0, 0], "b": [None, 0], "c": [1, 1]}[name]
    x = tc.stack_input(shape, 0)
    r = tc.check_stack(m, ops, x, tc.ref_run_op)
    print(f"stack {name}: compiled list in float64 at {r:.3f} of the bound")
    assert r <= 1
    # the whole module in one go, for the shape and the order of the layers
    with torch.no_grad():
        whole = _nhwc(m.double()(_nchw(x)))
    y = x
    for o in ops:
        y = tc.f32(tc.ref_run_op(o, y))
    assert y.shape == whole.shape and np.allclose(y, whole, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", sorted(tc.refused_stacks()))
def test_compile_stack_refuses(name):
    from roma_amd.tiny import _compile_stack
    with pytest.raises(NotImplementedError):
        _compile_stack(tc.refused_stacks()[name], "cpu")
