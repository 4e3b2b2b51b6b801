"""A caller's workspace need not be 256-byte aligned (MI355X): every operator that carves its workspace with Workspace256
(roma_amd/csrc/workspace.h) rounds the base up inside what it is given, and roma_op_*_workspace counts the 256 bytes that can
cost.  Each operator runs its smallest existing case twice through its Python wrapper - the workspace once at a 256-byte
aligned address and once 8 bytes past one, both times exactly roma_op_*_workspace bytes in the middle of a buffer of 0xFF
(tests/extents_cases.py) - and the outputs must be the same bits, the bytes around the workspace untouched.  The wrappers ask
torch.empty for their workspace; for the length of a run that one request is served from the guarded buffer.  Ordinary launches
on valid shapes: nothing here is meant to fault."""
import contextlib

import numpy as np
import pytest
import torch

from extents_cases import ALIGN, GUARD, POISON, assert_guards_intact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(x, dtype=np.float32):
    return torch.as_tensor(np.asarray(x, dtype=dtype), device=DEV)


@contextlib.contextmanager
def workspace_at(monkeypatch, lib, entries, skew):
    """inside the block a torch.empty of exactly the bytes that one of `entries` (roma_op_*_workspace) last returned, as uint8, is
    a view `skew` bytes past a 256-byte aligned address inside a 0xFF buffer with GUARD bytes on either side; yields the list
    of (backing, view) served"""
    sizes, held, real_empty = set(), [], torch.empty

    def spy(fn):
        def call(*args):
            n = fn(*args)
            sizes.add(int(n))
            return n
        return call

    def empty(*size, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list)) else size
        if kw.get("dtype") is torch.uint8 and len(shape) == 1 and int(shape[0]) in sizes and int(shape[0]) > 0:
            n = int(shape[0])
            backing = torch.full((GUARD + skew + n + GUARD + ALIGN,), POISON, dtype=torch.uint8, device=kw["device"])
            start = (-backing.data_ptr()) % ALIGN + GUARD + skew
            held.append((backing, backing[start:start + n]))
            return held[-1][1]
        return real_empty(*size, **kw)

    with monkeypatch.context() as m:
        for name in entries:
            m.setattr(lib, name, spy(getattr(lib, name)))
        m.setattr(torch, "empty", empty)
        yield held


def _bits(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    if isinstance(x, (tuple, list)):
        return tuple(_bits(v) for v in x)
    return x


# ---- the smallest case of every operator: name -> (its roma_op_*_workspace entries, a function that runs it and returns its outputs)
def _parent(case):
    def run():
        from ransac_parent_cases import CASES
        return CASES[case]()
    return run


def _relief():
    from test_cpu_geometry import relief_scene
    from test_gpu_essential import _normalised
    K, R, t, F, pa, pb, _ = relief_scene(n=300, outlier_frac=0.0, noise_px=0.3)
    return K, R, t, F, pa, pb, _normalised(pa, pb, K)


def _recover_pose():
    from roma_amd import recover_pose
    K, R, t, F, pa, pb, (x0, x1) = _relief()
    mask = np.random.default_rng(0).random(len(x0)) < 0.8
    return recover_pose(_dev(K.T @ F @ K, np.float64), _dev(x0), _dev(x1), _dev(mask, np.bool_))


def _refine_pose():
    from test_gpu_pose_refine import _refine_normalised
    K, R, t, F, pa, pb, (x0, x1) = _relief()
    return _refine_normalised(R, t, x0, x1, 1.0 / K[0, 0])


def _refine_model():
    from roma_amd import refine_fundamental
    K, R, t, F, pa, pb, _ = _relief()
    return refine_fundamental(_dev(F, np.float64), _dev(pa), _dev(pb), 1.0)


def _bundle_adjust():
    from roma_amd import bundle_adjust
    from test_gpu_bundle import _case
    s, X0, R0, t0, thr = _case("v2", False)
    return bundle_adjust(_dev(X0, np.float64), _dev(s["kpts"]), s["K"], _dev(R0, np.float64), _dev(t0, np.float64), thr, max_steps=3)


def _fuse_depth_maps():
    import depth_fusion_cases as dc
    from test_gpu_depth_fusion import _run
    return _run(dc.hand_made(), max_points=4, **dc.HAND_KW)


def _keypoints_from_matches():
    import set_keypoints_cases as sc
    from test_gpu_set_keypoints import _run
    return _run(sc.hand_made(), cell=2, radius=2.0, max_kpts=8)


def _build_tracks():
    import views_cases as vc
    from test_gpu_views import _tracks
    return _tracks(vc.hand_made())


def _render_points():
    import point_render_cases as pc
    from test_gpu_point_render import _run
    return _run(pc.hand_made())


OPS = {
    "ransac": (["roma_op_ransac_workspace"], _parent("H_count_256_refine1")),
    "magsac": (["roma_op_magsac_workspace"], _parent("F_magsac_256_lo3")),
    "essential": (["roma_op_essential_workspace"], _parent("E_count_256_K1")),
    "essential_magsac": (["roma_op_essential_magsac_workspace"], _parent("E_magsac_256_K0_lo3")),
    "absolute_pose": (["roma_op_absolute_pose_workspace"], _parent("ap_ragged_256")),
    "recover_pose": (["roma_op_recover_pose_workspace"], _recover_pose),
    "refine_pose": (["roma_op_refine_pose_workspace"], _refine_pose),
    "refine_model": (["roma_op_refine_model_workspace"], _refine_model),
    "bundle_adjust": (["roma_op_bundle_adjust_workspace"], _bundle_adjust),
    "fuse_depth_maps": (["roma_op_fuse_depth_maps_workspace"], _fuse_depth_maps),
    "keypoints_from_matches": (["roma_op_keypoints_from_matches_workspace"], _keypoints_from_matches),
    "build_tracks": (["roma_op_build_tracks_workspace"], _build_tracks),
    "render_points": (["roma_op_render_points_workspace"], _render_points),
}


@pytest.mark.parametrize("op", sorted(OPS))
def test_workspace_eight_bytes_past_alignment(built_lib, monkeypatch, op):
    entries, run = OPS[op]
    outs = []
    for skew in (0, 8):
        with workspace_at(monkeypatch, built_lib, entries, skew) as held:
            out = run()
            torch.cuda.synchronize()
        assert len(held) == 1, (op, skew, len(held))  # the wrapper's one workspace, and it was served from the guarded buffer
        backing, view = held[0]
        assert view.data_ptr() % ALIGN == skew
        assert_guards_intact(backing, view, f"{op}: workspace at +{skew}")
        outs.append(_bits(tuple(out)))
    assert len(outs[0]) > 0 and outs[0] == outs[1], op
