"""The operators' caller workspaces are sized and carved by one host-side carver (roma_amd/csrc/workspace.h).  The byte counts
of every roma_op_*_workspace entry are public: tests/golden/workspace_sizes.json records them as the build before the carver
returned them (tools/make_goldens.py workspace_sizes), and the in-tree build must return the same, row by row.
tests/workspace_check.cpp exercises the carver alone as a stand-alone program, compiled here with the host compiler."""
import json
import os
import subprocess

import pytest

from test_cpu_arena import _host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")))
ENTRIES = ("ransac", "magsac", "essential", "essential_magsac", "recover_pose", "refine_pose", "refine_model", "absolute_pose",
           "bundle_adjust", "build_tracks", "keypoints_from_matches", "fuse_depth_maps", "render_points", "sample_matches",
           "match_keypoints")


def test_golden_table_covers_every_entry():
    for entry in ENTRIES:
        rows = [r for r in ROWS if r["entry"] == entry]
        assert len(rows) >= 8, entry
        assert any(max(r["args"]) <= 2 and r["bytes"]["bf16"] > 0 for r in rows), entry  # all ones (two views where one is refused)
        refused = -1 if entry == "match_keypoints" else 0
        assert any(r["bytes"]["bf16"] == refused for r in rows), entry
        if entry != "fuse_depth_maps":  # B V H W < 2^31 there: 1 + 4 / 256 bytes a pixel stay below 2^32
            assert any(r["bytes"]["bf16"] > 1 << 32 for r in rows), entry
    assert {r["entry"] for r in ROWS} == set(ENTRIES)
    assert {r["args"][3] for r in ROWS if r["entry"] == "sample_matches"} == {0, 1}


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_workspace_bytes_are_the_parents(fmt):
    from roma_amd import _lib
    lib = _lib.load(fmt)
    for r in ROWS:
        got = getattr(lib, f"roma_op_{r['entry']}_workspace")(*r["args"])
        assert got == r["bytes"][fmt], (r, got)


def test_carver_sizing_and_live_runs_agree(tmp_path):
    cxx = _host_cxx()
    assert cxx, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / "workspace_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "roma_amd", "csrc"),
                         os.path.join(ROOT, "tests", "workspace_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=30)
    assert out.returncode == 0 and out.stdout.strip() == "workspace ok", out.stdout + out.stderr


def test_sixteen_byte_policy_still_refuses_a_workspace_at_plus_8(built_lib):
    """sample_matches and match_keypoints use their workspace as given: no slack to align it in, so + 8 is refused as before
    (host validation: no address here is ever read)."""
    lib = built_lib
    p = 1 << 20
    need = lib.roma_op_sample_matches_workspace(2, 1000, 100, 1)
    args = lambda ws: (p, p, p, 2, 1000, 100, 1, 0.05, 1, p, p, None, None, None, None, ws, need, None)  # noqa: E731
    assert lib.roma_op_sample_matches(*args(p + 8)) != 0
    assert lib.roma_last_error() == b"sample_matches: matches, out_matches and workspace must be 16-byte aligned"
    assert lib.roma_op_sample_matches(*args(p)[:16], need - 1, None) != 0
    assert lib.roma_last_error() == b"sample_matches: workspace too small (roma_op_sample_matches_workspace)"

    B, NA, NB, H, W = 2, 100, 90, 8, 12
    need = lib.roma_op_match_keypoints_workspace(B, NA, NB)
    args = lambda ws, n: (p, p, p, p, p, H * W * 4, W * 4, p, H * W, W, None, 0, B, NA, NB, H, W, 0.005, 0.0, 50, p, p, p, p, p, ws,  # noqa: E731
                          n, None)
    assert lib.roma_op_match_keypoints(*args(p + 8, need)) != 0
    assert lib.roma_last_error() == b"match_keypoints: warp and workspace must be 16-byte aligned"
    assert lib.roma_op_match_keypoints(*args(p, need - 1)) != 0
    assert lib.roma_last_error() == b"match_keypoints: workspace is too small (roma_op_match_keypoints_workspace)"
