"""Build-container only: record what the UNMODIFIED reference makes of the scene of tests/gt_warp_cases.py in
tests/golden/gt_warp_reference.npz - inputs (in_*) and recorded outputs (ref_*) only, no reference program text.

    python tools/make_gt_warp_goldens.py

Runs on the CPU in float64, as the reference's dense benchmark does: romatch/utils/utils.py warp_kpts (both return forms) and
get_gt_warp (with the x1_n grid it builds, caught at its call of warp_kpts), and
romatch/benchmarks/megadepth_dense_benchmark.py MegadepthDenseBenchmark.geometric_dist.  The benchmark module imports the data
loaders, some of whose dependencies (h5py, kornia, ...) are absent here; empty stand-ins let the import pass - geometric_dist calls none."""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402


ABSENT = ("h5py", "kornia", "tqdm", "poselib", "albumentations", "einops", "matplotlib", "wandb")


class _Absent(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """empty stand-ins for the data loaders' dependencies that are not installed: any attribute is a placeholder class"""

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in ABSENT:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        mod = types.ModuleType(spec.name)
        mod.__path__ = []
        mod.__getattr__ = lambda attr: type(attr, (), {})
        return mod

    def exec_module(self, module):
        pass


def _reference():
    ref_import.install_stubs()
    sys.meta_path.append(_Absent())  # after the real finders: only what is missing
    import romatch.utils.utils as U
    import romatch.benchmarks.megadepth_dense_benchmark as MB
    return U, MB


def main():
    import gt_warp_cases as cases
    U, MB = _reference()
    s = cases.build_scene()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items()}
    args = (t["depth0"].double(), t["depth1"].double(), t["T"], t["K0"], t["K1"])
    kp = t["kpts"].double()
    out = {"in_" + k: v for k, v in s.items()}
    valid, warped = U.warp_kpts(kp, *args, relative_depth_error_threshold=cases.THRESHOLD)
    rel, warped2 = U.warp_kpts(kp, *args, return_relative_depth_error=True, relative_depth_error_threshold=cases.THRESHOLD)
    assert torch.equal(warped, warped2)
    out["ref_valid"], out["ref_warped"], out["ref_rel"] = valid.numpy(), warped.numpy(), rel.numpy()

    # get_gt_warp and the grid it hands to warp_kpts (float32 depths, as a data loader yields them)
    caught = {}
    inner = U.warp_kpts

    def spy(kpts0, *a, **kw):
        caught["x1_n"] = kpts0.detach().clone()
        return inner(kpts0, *a, **kw)
    U.warp_kpts = spy
    try:
        x2, prob = U.get_gt_warp(t["depth0"], t["depth1"], t["T"], t["K0"], t["K1"], relative_depth_error_threshold=cases.THRESHOLD)
    finally:
        U.warp_kpts = inner
    out["ref_gt_x2"], out["ref_gt_prob"], out["ref_gt_x1_n"] = x2.numpy(), prob.numpy(), caught["x1_n"].numpy()
    assert out["ref_gt_x1_n"].dtype == np.float64 and x2.dtype == torch.float64 and prob.dtype == torch.float32

    # geometric_dist per batch (B pairs) and per pair
    gd, p1, p3, p5, gprob = MB.MegadepthDenseBenchmark.geometric_dist(None, t["depth0"], t["depth1"], t["T"], t["K0"], t["K1"], t["matches"])
    out["ref_gd"], out["ref_pck"], out["ref_prob"] = gd.numpy(), np.array([float(p1), float(p3), float(p5)]), gprob.numpy()
    assert gd.dtype == torch.float64
    np.savez_compressed(cases.GOLDEN_FILE, **out)
    size = os.path.getsize(cases.GOLDEN_FILE)
    print(f"{cases.GOLDEN_FILE}: {size} bytes; valid rows per pair {valid.sum(dim=1).tolist()}, ", end="")
    print(f"epe {float(gd.mean()):.4f} pck {out['ref_pck']} over {gd.numel()} valid pixels")
    assert size < 256 * 1024


if __name__ == "__main__":
    main()
