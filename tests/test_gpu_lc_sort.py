"""The atomic-free counting sort of the incoherent tiles' queries (local_corr.hip: band histograms in LDS, one scan, LDS
cursors) against the device-atomic sort it replaces and against per-query gathers, through roma_op_local_corr_window on the
16-bit library.  lc_bin: 1 = the new sort, 2 = the atomic sort, 0 = per-query gathers.

Sizes: (19, 21) odd edges on both axes; (24, 40) three tile rows, so a band of the sort holds more than one; (16, 16) with
every query at one point: 256 queries of one bin = 4 full items.  (19, 21) at one point: 399 queries = 6 items + 15.
(72, 24): nine tile rows = five bands per image, so the prefix over the earlier bands has more than one term.
A query's result does not depend on its place in the sorted list, so the two sorts must agree bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
B, CH = 2, 64
SIZES = [(19, 21), (24, 40), (16, 16), (72, 24)]
RADII = [2, 3, 7]
WARPS = ["uniform", "one_point", "half_identity"]


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available()
    return built_lib


def _warp(kind, h, w):
    g = np.random.Generator(np.random.PCG64(1000 * h + w))
    if kind == "uniform":  # every tile incoherent, some windows wholly outside the image (|coordinate| up to 1.3)
        return torch.from_numpy(g.uniform(-1.3, 1.3, size=(B, h * w, 2)).astype(np.float32))
    if kind == "one_point":  # a single bin per image
        return torch.tensor([0.21, -0.37]).repeat(B, h * w, 1).contiguous()
    ys, xs = torch.meshgrid((torch.arange(h) + 0.5) * 2 / h - 1, (torch.arange(w) + 0.5) * 2 / w - 1, indexing="ij")
    wp = torch.stack((xs, ys), dim=-1).reshape(1, h * w, 2).repeat(B, 1, 1)
    rand = torch.from_numpy(g.uniform(-1.0, 1.0, size=(B, h * w, 2)).astype(np.float32))
    bottom = (torch.arange(h * w) // w >= h // 2)[None, :, None]
    return torch.where(bottom, rand, wp).contiguous()  # identity on the top half (coherent tiles), random below


_CASES = {}


def _case(h, w, kind):
    """inputs of a (size, warp) pair, made once and shared by the radii"""
    key = (h, w, kind)
    if key not in _CASES:
        g = np.random.Generator(np.random.PCG64(7 + h * 64 + w))
        f0 = torch.from_numpy(g.standard_normal(size=(B, h * w, CH), dtype=np.float32)).bfloat16().cuda()
        f1 = torch.from_numpy(g.standard_normal(size=(B, h * w, CH), dtype=np.float32)).bfloat16().cuda()
        _CASES[key] = (f0, f1, _warp(kind, h, w).cuda())
    return _CASES[key]


def _run(lib, f0, f1, warp, h, w, r, ws=None):
    K = (2 * r + 1) ** 2
    out = torch.full((B, h * w, K), float("nan"), device="cuda")
    args = (C.c_void_p(f0.data_ptr()), C.c_void_p(f1.data_ptr()), C.c_void_p(warp.data_ptr()), C.c_void_p(out.data_ptr()),
            B, h, w, CH, r, CH ** -0.5, K, BF16, F32)
    if ws is None:
        rc = lib.roma_op_local_corr_window(*args, None)
    else:
        rc = lib.roma_op_local_corr_window_ws(*args, C.c_void_p(ws.data_ptr()), ws.numel() * 4, None)
    assert rc == 0, lib.roma_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_workspace_entry_takes_no_scratch_where_none_is_needed(lib):
    """radius 1 runs the per-pixel kernel: the workspace size is 0 and the caller-owned-scratch entry accepts NULL"""
    h, w, r = 19, 21, 1
    f0, f1, warp = _case(h, w, "uniform")
    assert lib.roma_op_local_corr_window_workspace(B, h, w, r) == 0
    K = (2 * r + 1) ** 2
    outs = []
    for with_ws in (False, True):
        out = torch.full((B, h * w, K), float("nan"), device="cuda")
        args = (C.c_void_p(f0.data_ptr()), C.c_void_p(f1.data_ptr()), C.c_void_p(warp.data_ptr()), C.c_void_p(out.data_ptr()),
                B, h, w, CH, r, CH ** -0.5, K, BF16, F32)
        rc = lib.roma_op_local_corr_window_ws(*args, None, 0, None) if with_ws else lib.roma_op_local_corr_window(*args, None)
        assert rc == 0, lib.roma_last_error().decode()
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("kind", WARPS)
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("r", RADII)
def test_lds_sort_matches_atomic_sort_and_gathers(lib, r, h, w, kind):
    f0, f1, warp = _case(h, w, kind)
    tiles = B * ((h + 7) // 8) * ((w + 7) // 8)
    outs = {}
    try:
        # the classifier calls a tile coherent when the rectangle of its windows, clipped to the image, fits the tile kernel's
        # stage (320 pixels for r <= 3, 704 for r = 7): windows that all start at one point always do, and so does every tile of
        # an image that small - the sort would see nothing.  lc_mode = 1 puts every tile on the incoherent list; the mixed
        # warp keeps the classifier's own decision.
        if kind != "half_identity":
            assert lib.roma_tuning(b"lc_mode", 1) == 0
        for mode in (1, 2, 0):
            assert lib.roma_tuning(b"lc_bin", mode) == 0
            outs[mode] = _run(lib, f0, f1, warp, h, w, r)
        # caller-owned scratch, poisoned: a slot of the item list or of a table that is read without having been written shows
        # up as a missing query (the poison is negative, i.e. padding: the query's output stays NaN) or as a wrong count (the
        # queries of a bin then land in a neighbour's slots)
        assert lib.roma_tuning(b"lc_bin", 1) == 0
        nbytes = lib.roma_op_local_corr_window_workspace(B, h, w, r)
        assert nbytes > 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4,), -2, dtype=torch.int32, device="cuda")
        outs["poisoned"] = _run(lib, f0, f1, warp, h, w, r, ws)
        n_incoherent, _, n_items, _ = ws[:4].tolist()  # header of the scratch (local_corr.hip): tiles on the incoherent list, items
    finally:
        lib.roma_tuning(b"lc_bin", -1)
        lib.roma_tuning(b"lc_mode", -1)
    # the sort really saw what the case is about: the tiles on the incoherent list, and for the single-bin warp every image as
    # ceil(h w / 64) items of one bin (16 x 16: 4 full items, no padding; 19 x 21: 6 items + 15 queries)
    if kind == "uniform":
        assert n_incoherent == tiles and n_items >= B * ((h * w + 63) // 64)
    elif kind == "one_point":
        assert n_incoherent == tiles and n_items == B * ((h * w + 63) // 64)
    elif h * w <= (320 if r <= 3 else 704):  # the whole image fits the stage: no incoherent tile, the sort launches return at once
        assert n_incoherent == 0 and n_items == 0
    else:
        assert 0 < n_incoherent < tiles and n_items > 0
    assert np.isfinite(outs[1]).all()
    assert np.array_equal(outs[1], outs[2])
    assert np.array_equal(outs[1], outs["poisoned"])
    # sorted items on the matrix core against per-query dot products: exact products, f32 sums in another order - the bound of
    # tests/test_gpu_ops.py::test_local_corr_tiled_gather_and_legacy_paths_agree for the 16-bit forms
    assert np.allclose(outs[1], outs[0], atol=2e-5, rtol=1e-5), float(np.abs(outs[1] - outs[0]).max())
