"""The numpy oracle of point-cloud rendering - tools/point_render_ref.py against a hand-made case whose maps are written out, against
a scalar restatement of the definition, and for its properties - the margins of every case the GPU file compares bit for bit,
roma_amd.orbit_cameras, and the C ABI of roma_op_render_points without a GPU (argument validation only)."""
import glob
import math
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import ROOT
from point_render_cases import (HAND_RAW_INDEX, OFF, check_hand_made, gpu_margins, hand_made, prr, random_case, random_cut, random_kw, random_ref,
                                RANDOM_PARAMS, ref)

NEW_SYMBOLS = ["roma_op_render_points", "roma_op_render_points_workspace"]
f32 = np.float32
EMPTY = (1 << 64) - 1


def _depth_of(key):
    return struct.unpack("<f", struct.pack("<I", key >> 32))[0]


def scalar_render(c, radius=1, near=1e-6, far=math.inf, occlusion_radius=2, occlusion_rel=0.05, occlusion_count=3, fill_radius=1, fill_min=3,
                  background=(0, 0, 0)):
    """the definition again, row by row and pixel by pixel in Python floats and integers"""
    pts, K, R, t, H, W = c["points"], c["cameras"], c["R"], c["t"], c["H"], c["W"]
    N = len(pts)
    cnt = N if c["count"] is None else min(max(c["count"], 0), N)
    Cn = len(K)
    depth = np.full((Cn, H, W), np.nan, dtype=f32)
    index = np.full((Cn, H, W), -1, dtype=np.int32)
    mask = np.zeros((Cn, H, W), dtype=np.uint8)
    stats = np.zeros((Cn, 4), dtype=np.int32)
    for k in range(Cn):
        fx, fy, cx, cy = (float(x) for x in (K[k][0, 0], K[k][1, 1], K[k][0, 2], K[k][1, 2]))
        Rk, tk = [[float(x) for x in row] for row in R[k]], [float(x) for x in t[k]]
        key = [[EMPTY] * W for _ in range(H)]
        for n in range(cnt):
            X = [float(x) for x in pts[n]]
            if not all(math.isfinite(x) for x in X):
                continue
            y = [((Rk[i][0] * X[0] + Rk[i][1] * X[1]) + Rk[i][2] * X[2]) + tk[i] for i in range(3)]
            if not near <= y[2] <= far:
                continue
            with np.errstate(over="ignore"):
                zf = float(f32(y[2]))
            u, v = fx * (y[0] / y[2]) + cx, fy * (y[1] / y[2]) + cy
            if not (math.isfinite(zf) and zf > 0 and math.isfinite(u) and math.isfinite(v)):
                continue
            c0, r0 = math.floor(u), math.floor(v)
            if not (-radius <= c0 < W + radius and -radius <= r0 < H + radius):
                continue
            stats[k, 0] += 0 <= r0 < H and 0 <= c0 < W
            mine = (struct.unpack("<I", struct.pack("<f", zf))[0] << 32) | n
            for r in range(max(r0 - radius, 0), min(r0 + radius, H - 1) + 1):
                for col in range(max(c0 - radius, 0), min(c0 + radius, W - 1) + 1):
                    key[r][col] = min(key[r][col], mine)
        removed = [[False] * W for _ in range(H)]
        for r in range(H):
            for col in range(W):
                if key[r][col] == EMPTY or occlusion_radius == 0:
                    continue
                z, nearer = _depth_of(key[r][col]), 0
                for rr in range(max(r - occlusion_radius, 0), min(r + occlusion_radius, H - 1) + 1):
                    for cc in range(max(col - occlusion_radius, 0), min(col + occlusion_radius, W - 1) + 1):
                        nearer += key[rr][cc] != EMPTY and z > _depth_of(key[rr][cc]) * (1.0 + occlusion_rel)
                removed[r][col] = nearer >= occlusion_count
        for r in range(H):
            for col in range(W):
                hit = key[r][col] != EMPTY
                final, filled = (key[r][col] if hit and not removed[r][col] else EMPTY), False
                if final == EMPTY and fill_radius > 0:
                    alive = [key[rr][cc] for rr in range(max(r - fill_radius, 0), min(r + fill_radius, H - 1) + 1)
                             for cc in range(max(col - fill_radius, 0), min(col + fill_radius, W - 1) + 1)
                             if key[rr][cc] != EMPTY and not removed[rr][cc]]
                    if len(alive) >= fill_min:
                        final, filled = min(alive), True
                mask[k, r, col] = hit * 1 + removed[r][col] * 2 + filled * 4
                if final != EMPTY:
                    depth[k, r, col], index[k, r, col] = _depth_of(final), final & 0xFFFFFFFF
        stats[k, 1:] = (mask[k] & 1).sum(), ((mask[k] >> 1) & 1).sum(), ((mask[k] >> 2) & 1).sum()
    return {"depth": depth, "index": index, "mask": mask, "stats": stats}


def _same_as_scalar(c, **kw):
    o, s = ref(c, **kw), scalar_render(c, **{k: v for k, v in dict(c["kw"], **kw).items()})
    assert np.array_equal(o["depth"].view(np.int32), s["depth"].view(np.int32))
    for k in ("index", "mask", "stats"):
        assert np.array_equal(o[k], s[k]), k
    return o


def test_restatement_on_the_hand_made_case():
    """two rows in a pixel at different depths, two at the same float32 depth, a row behind the camera, one beyond far, one outside the
    frustum whose splat reaches the border and one out of reach, a splat clipped at a corner, a NaN row, a row beyond count, and one
    see-through pixel the filter removes and the fill closes: point_render_cases.HAND_EXPECTED spells every pixel out"""
    o = ref(hand_made())
    assert np.array_equal((o["key"][0] & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32), np.asarray(HAND_RAW_INDEX))
    assert float(prr.key_depth(o["key"][0])[2, 3]) == 4.0
    check_hand_made(o)
    _same_as_scalar(hand_made())


@pytest.mark.parametrize("radius,flt,fil", [(0, "off", "off"), (1, "o2c3", "f1m3"), (2, "o2c1", "f1m3"), (1, "o2c1", "off")])
def test_restatement_equals_the_scalar_definition(radius, flt, fil):
    o = _same_as_scalar(random_cut(), **random_kw(radius, flt, fil))
    assert (o["stats"][:, 1] > 500).all() and ((o["stats"][:, 2] > 0).all() or flt == "off")


@pytest.mark.parametrize("radius,flt,fil", RANDOM_PARAMS)
def test_random_case_exercises_the_filter_and_the_fill(radius, flt, fil):
    st = random_ref(radius, flt, fil)["stats"]
    assert (st[:, 0] > 5000).all() and (st[:, 1] > 2000).all()
    assert ((st[:, 2] > 0).all() if flt != "off" else not st[:, 2].any()), "with the filter on some pixels are removed"
    assert ((st[:, 3] > 0).all() if fil != "off" else not st[:, 3].any()), "with the fill on some pixels are filled"


def test_a_frame_does_not_depend_on_the_other_frames():
    c = random_case()
    o = random_ref(1, "o2c3", "f1m3")
    for k in range(3):
        one = ref(dict(c, cameras=c["cameras"][k:k + 1], R=c["R"][k:k + 1], t=c["t"][k:k + 1]), **random_kw(1, "o2c3", "f1m3"))
        for name in ("depth", "index", "color", "mask", "stats", "key"):
            assert np.array_equal(one[name][0], o[name][k], equal_nan=True), (k, name)


def test_permuting_rows_of_different_depth_changes_only_index():
    """the rows of the cut whose float32 depth in a camera is shared with no other row: their order cannot matter but for `index`"""
    c = random_cut()
    pts = c["points"]
    keep = np.isfinite(pts).all(axis=1)
    for k in range(3):
        with np.errstate(all="ignore"):
            z = (pts.astype(np.float64) @ c["R"][k].T + c["t"][k])[:, 2].astype(f32)
        _, first, cnt = np.unique(z, return_index=True, return_counts=True)
        single = np.zeros(len(pts), dtype=bool)
        single[first[cnt == 1]] = True
        keep &= single
    rows = np.nonzero(keep)[0]
    assert len(rows) > 1500
    perm = np.random.default_rng(3).permutation(len(rows))
    a = dict(c, points=pts[rows], colors=c["colors"][rows])
    b = dict(c, points=pts[rows][perm], colors=c["colors"][rows][perm])
    oa, ob = ref(a, **random_kw(1, "o2c3", "f1m3")), ref(b, **random_kw(1, "o2c3", "f1m3"))
    for name in ("depth", "color", "mask", "stats"):
        assert np.array_equal(oa[name], ob[name], equal_nan=True), name
    have = oa["index"] >= 0
    assert np.array_equal(have, ob["index"] >= 0) and np.array_equal(oa["index"][have], perm[ob["index"][have]])
    assert not np.array_equal(oa["index"], ob["index"])


def test_plain_z_buffer_holds_every_usable_row():
    """radius 0, both passes off: every usable row whose cell lies inside the image satisfies depth[cell] <= fl32(z)"""
    c = random_case()
    o = ref(c, radius=0, **OFF)
    X = c["points"].astype(np.float64)
    checked = 0
    with np.errstate(all="ignore"):
        for k in range(3):
            R, t, K = c["R"][k], c["t"][k], c["cameras"][k]
            y = [((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i] for i in range(3)]
            u, v = K[0, 0] * (y[0] / y[2]) + K[0, 2], K[1, 1] * (y[1] / y[2]) + K[1, 2]
            ok = np.isfinite(c["points"]).all(axis=1) & (y[2] >= 1e-6) & (u >= 0) & (u < c["W"]) & (v >= 0) & (v < c["H"])
            cell = o["depth"][k][np.floor(v[ok]).astype(int), np.floor(u[ok]).astype(int)]
            assert np.isfinite(cell).all() and (cell <= y[2][ok].astype(f32)).all()
            assert int(ok.sum()) == o["stats"][k, 0]
            checked += int(ok.sum())
    assert checked > 20000


def test_margins_of_every_case_the_gpu_file_compares():
    """no float decision of the restatement - the floor that picks a cell, near / far, the frustum bounds, the occlusion test - lies
    within 1e-9 (relative) of its threshold in any case tests/test_gpu_point_render.py compares bit for bit: a mismatch there is a
    defect, not a borderline case"""
    seen = 0
    for name, m in gpu_margins():
        seen += 1
        worst = min(m, key=m.get)
        print(f"{name}: smallest margin {m[worst]:.3e} ({worst})")
        for k, x in m.items():
            assert x > 1e-9, (name, k, x)
    assert seen == 1 + len(RANDOM_PARAMS) + 2 + 1 + 6


def test_orbit_cameras():
    from roma_amd import orbit_cameras
    c = random_case()
    R0, t0, centre = c["R"][1], c["t"][1], np.array([0.3, -0.2, 5.0])
    angles = [0.0, 0.4, -1.1, math.pi, 2.5]
    for axis in ((0.0, 1.0, 0.0), (0.3, 2.0, -0.5)):
        R, t = orbit_cameras(R0, t0, centre, angles, axis=axis, device="cpu")
        assert R.dtype == torch.float64 and tuple(R.shape) == (5, 3, 3) and tuple(t.shape) == (5, 3)
        R, t = R.numpy(), t.numpy()
        assert np.array_equal(R[0].view(np.int64), R0.view(np.int64)) and np.array_equal(t[0].view(np.int64), t0.view(np.int64))
        for k in range(5):
            assert np.allclose(R[k] @ R[k].T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R[k]) - 1.0) < 1e-14
            assert np.allclose(R[k] @ centre + t[k], R0 @ centre + t0, atol=1e-13)  # the centre keeps its place, its depth with it
        # the camera centre turns about the axis through `centre` by the angle
        a = np.asarray(axis) / np.linalg.norm(axis)
        c0, c1 = -R0.T @ t0 - centre, -R[1].T @ t[1] - centre
        assert abs(c0 @ a - c1 @ a) < 1e-13 and abs(np.linalg.norm(c0) - np.linalg.norm(c1)) < 1e-13
        p0, p1 = c0 - (c0 @ a) * a, c1 - (c1 @ a) * a
        assert abs(math.atan2(np.cross(p0, p1) @ a, p0 @ p1) - 0.4) < 1e-12
    for bad in (lambda: orbit_cameras(np.eye(2), t0, centre, angles, device="cpu"), lambda: orbit_cameras(R0, t0, centre, [], device="cpu"),
                lambda: orbit_cameras(R0, t0, centre, angles, axis=(0, 0, 0), device="cpu"),
                lambda: orbit_cameras(R0, t0, centre, [math.nan], device="cpu")):
        with pytest.raises(ValueError):
            bad()


def test_abi_symbols_and_sources(built_lib):
    from roma_amd import _lib
    header = open(os.path.join(ROOT, "include", "roma_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES
        for fmt in ("bf16", "f16"):
            assert hasattr(_lib.load(fmt), name)
        # the header documents the entry and the table's arity is the prototype's
        proto = re.search(rf"^(?:int|long) {name}\(([^;]*)\);", header, re.M | re.S)
        assert proto and len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [29, 4]
    doc = header[header.index("/* Point-cloud rendering"):header.index("long roma_op_render_points_workspace")]
    for word in ("tools/point_render_ref.py", "occlusion_count", "fill_min", "grows by up to o + f", "Refused before anything is enqueued"):
        assert word in doc, word
    mk = open(os.path.join(ROOT, "roma_amd", "csrc", "Makefile")).read()
    assert "point_render.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "point_render" not in re.search(r"^PK_SRCS = (.*)$", mk, re.M).group(1).split()
    ws = built_lib.roma_op_render_points_workspace
    assert ws(0, 3, 48, 64) == 0 and ws(1, 0, 48, 64) == 0 and ws(1, 3, 0, 64) == 0 and ws(1, 3, 48, 0) == 0 and ws(256, 256, 8, 8) == 0
    assert ws(1, 1, 26755, 26755) == 0 and ws(2, 30, 3000, 4000) == 0  # 3 B C H W >= 2^31
    assert 0 < ws(1, 3, 48, 64) < ws(1, 3, 480, 640) < ws(4, 3, 480, 640)
    assert ws(1, 60, 864, 1152) >= 9 * 60 * 864 * 1152  # 8 bytes a pixel for the key and one for the decision


def test_c_abi_validates_before_device_work(built_lib):
    lib = built_lib
    p = 16  # any non-null aligned address: validation must fail before it is used
    need = lib.roma_op_render_points_workspace(2, 3, 48, 64)
    inf = math.inf

    def rp(points=p, colors=None, cam=p, R=p, t=p, B=2, N=100, Cn=3, H=48, W=64, radius=1, near=1e-6, far=inf, o=2, rel=0.05, oc=3, f=1, fm=3,
           bg=0, color=None, depth=p, index=p, mask=p, stats=p, ws=p, nws=need):
        return lib.roma_op_render_points(points, colors, None, None, cam, R, t, B, N, Cn, H, W, radius, near, far, o, rel, oc, f, fm, bg, color,
                                         depth, index, mask, stats, ws, nws, None)

    cases = [(lambda: rp(points=None), "null pointer"), (lambda: rp(cam=None), "null pointer"), (lambda: rp(R=None), "null pointer"),
             (lambda: rp(t=None), "null pointer"), (lambda: rp(depth=None), "null pointer"), (lambda: rp(index=None), "null pointer"),
             (lambda: rp(mask=None), "null pointer"), (lambda: rp(stats=None), "null pointer"), (lambda: rp(colors=p), "go together"),
             (lambda: rp(color=p), "go together"), (lambda: rp(Cn=0), "C >= 1"), (lambda: rp(B=-1), "B must"),
             (lambda: rp(B=21846), "65535"), (lambda: rp(H=0), "positive"), (lambda: rp(W=0), "positive"), (lambda: rp(N=-1), "N must"),
             (lambda: rp(radius=-1), "[0, 4]"), (lambda: rp(radius=5), "[0, 4]"), (lambda: rp(o=-1), "[0, 4]"), (lambda: rp(o=5), "[0, 4]"),
             (lambda: rp(f=-1), "[0, 4]"), (lambda: rp(f=5), "[0, 4]"), (lambda: rp(oc=0), "at least 1"), (lambda: rp(fm=0), "at least 1"),
             (lambda: rp(rel=-0.1), "occlusion_rel"), (lambda: rp(rel=math.nan), "occlusion_rel"), (lambda: rp(near=0.0), "near"),
             (lambda: rp(near=-1.0), "near"), (lambda: rp(near=math.nan), "near"), (lambda: rp(near=2.0, far=1.0), "far"),
             (lambda: rp(far=math.nan), "far"), (lambda: rp(bg=-1), "background"), (lambda: rp(bg=1 << 24), "background"),
             (lambda: rp(B=1, Cn=1, H=26755, W=26755), "2^31"), (lambda: rp(B=2, Cn=30, H=3000, W=4000), "2^31"),
             (lambda: rp(nws=need - 1), "workspace too small"), (lambda: rp(ws=None), "workspace too small")]
    for k, (call, word) in enumerate(cases):
        assert call() != 0 and word in lib.roma_last_error().decode(), (k, word, lib.roma_last_error())
    assert rp(B=0) == 0 and rp(B=0, ws=None, nws=0) == 0  # nothing to do: no launch, no error
    assert rp(far=inf, nws=need - 1) != 0  # +inf is allowed: the refusal is the workspace's
    assert "workspace" in lib.roma_last_error().decode()


def test_python_argument_errors(built_lib):
    """every shape and value check of render_points raises before a device is asked for: the tensors here live on the host, and a
    call that passes the checks ends at `no CPU fallback`"""
    import roma_amd
    from roma_amd._lib import RomaHipError
    pts, col, cnt = torch.zeros((2, 10, 3)), torch.zeros((2, 10, 3), dtype=torch.uint8), torch.tensor([3, 4])
    K, R, t = np.eye(3), torch.eye(3).expand(2, 4, 3, 3), torch.zeros(2, 4, 3)
    rp = roma_amd.render_points
    for call in (lambda: rp(pts, K, R, t, 8, 8, colors=col, counts=cnt), lambda: rp(pts[0], K, R[0], t[0], 8, 8), lambda: rp(pts, K, R[0], t[0], 8, 8)):
        with pytest.raises(RomaHipError, match="no CPU fallback"):
            call()
    bad = [lambda: rp(pts[..., :2], K, R, t, 8, 8), lambda: rp(pts[0, 0], K, R, t, 8, 8), lambda: rp(pts[0], K, R, t, 8, 8),
           lambda: rp(pts, K, R[:1], t[:1], 8, 8), lambda: rp(pts, K, R, t[:, :3], 8, 8), lambda: rp(pts, K, R[..., :2], t, 8, 8),
           lambda: rp(pts, K, R[:, :0], t[:, :0], 8, 8), lambda: rp(pts, None, R, t, 8, 8), lambda: rp(pts, np.zeros((3, 3, 3)), R, t, 8, 8),
           lambda: rp(pts, K, R, t, 0, 8), lambda: rp(pts, K, R, t, 8, 0), lambda: rp(pts, K, R, t, 20000, 20000),
           lambda: rp(pts, K, R, t, 8, 8, colors=col[:, :5]), lambda: rp(pts, K, R, t, 8, 8, colors=col.float()),
           lambda: rp(pts, K, R, t, 8, 8, counts=cnt[:1]), lambda: rp(pts, K, R, t, 8, 8, counts=cnt.float()),
           lambda: rp(pts, K, R, t, 8, 8, radius=5), lambda: rp(pts, K, R, t, 8, 8, radius=-1), lambda: rp(pts, K, R, t, 8, 8, occlusion_radius=5),
           lambda: rp(pts, K, R, t, 8, 8, fill_radius=-1), lambda: rp(pts, K, R, t, 8, 8, occlusion_count=0), lambda: rp(pts, K, R, t, 8, 8, fill_min=0),
           lambda: rp(pts, K, R, t, 8, 8, occlusion_rel=-1.0), lambda: rp(pts, K, R, t, 8, 8, occlusion_rel=math.nan),
           lambda: rp(pts, K, R, t, 8, 8, near=0.0), lambda: rp(pts, K, R, t, 8, 8, near=2.0, far=1.0), lambda: rp(pts, K, R, t, 8, 8, far=math.nan),
           lambda: rp(pts, K, R, t, 8, 8, background=(0, 0)), lambda: rp(pts, K, R, t, 8, 8, background=(0, 0, 256)),
           lambda: rp(torch.zeros((300, 4, 3)), K, torch.eye(3).expand(300, 300, 3, 3), torch.zeros(300, 300, 3), 8, 8)]
    for k, call in enumerate(bad):
        try:
            call()
        except ValueError:
            continue
        pytest.fail(f"bad call {k} raised no ValueError")
    for name in ("render_points", "orbit_cameras", "PointRender"):
        assert name in roma_amd.__all__ and hasattr(roma_amd, name)
    assert callable(roma_amd.RegressionMatcher.render_fusion)


@pytest.mark.parametrize("build", ["build", "build_f16"])
def test_point_render_kernels_have_no_spills_and_no_scratch(build):
    obj = os.path.join(ROOT, "roma_amd", "csrc", build, "point_render.o")
    if not glob.glob(obj):
        pytest.skip(f"{build}/point_render.o not built")
    import kernel_resources
    ks = kernel_resources.kernels(obj)
    names = sorted(re.sub(r"roma::|\(anonymous namespace\)::", "", k["name"]) for k in ks)
    assert names == ["render_fill_kernel", "render_filter_kernel", "render_splat_kernel"], names
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] <= 256, k
        assert k["vgpr"] <= 64, k  # eight waves a SIMD: the splat hides the latency of its atomics with occupancy alone
