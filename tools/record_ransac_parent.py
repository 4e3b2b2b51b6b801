"""Records tests/golden/ransac_parent.npz, the fixture of tests/test_gpu_ransac_parent.py: every output tensor (model or R and t,
mask, ok, info, and the score where the scoring has one) of every case of tests/ransac_parent_cases.py, through the public
Python API.  Run it on the GPU from a checkout of the commit whose bits are to be kept - the parent of the change under
test - never from the tree the test then runs on.  Key "<case>/<i>": output i of the case.
Usage: python tools/record_ransac_parent.py [--out tests/golden/ransac_parent.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ransac_parent_cases import CASES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ransac_parent.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_ransac_parent: no HIP device (there is no CPU fallback)")
    arrays = {}
    for name, run in sorted(CASES.items()):
        out = run()
        for i, x in enumerate(out):
            arrays[f"{name}/{i}"] = x.cpu().numpy()
        info = out[4 if name.startswith("ap_") else 3].cpu().numpy()
        print(f"{name}: {len(out)} outputs, rounds {info[:, 0].tolist()}, ok {out[3 if name.startswith('ap_') else 2].cpu().tolist()}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print(f"{len(arrays)} arrays of {len(CASES)} cases -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
