"""Build-container only: record what torch's grid_sample and the UNMODIFIED reference's tensor_to_pil make of the scene of
tests/morph_cases.py in tests/golden/morph_reference.npz - inputs (in_*) and recorded outputs (ref_*) only, no reference program text.

    python tools/make_morph_goldens.py

The reference's demo/demo_3D_effect.py keeps its frame loop under `if __name__ == "__main__"`, so it cannot be imported; the loop
below restates it: for every t the Python scalars (1 - t) and t multiply the two halves of the float32 warp, F.grid_sample
(bilinear, align_corners=False) samples image B, and romatch.utils.utils.tensor_to_pil turns the frame into 8 bits.  For the
certainty blend the frame goes through visualize_warp's `white_im * (1 - certainty) + certainty * warp_im` first.  Runs on the CPU
in float32.  Asserts that the share of values the uint8 comparison rule excuses stays below its cap."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402


def frames(tensor_to_pil, warp, image, ts, certainty=None, background=1.0):
    """one pair: (float frames [T, 3, H, W], uint8 frames [T, H, W, 3])"""
    coords_a, coords_b = warp[..., :2], warp[..., 2:]
    fl, u8 = [], []
    for t in ts:
        t = float(t)
        grid = (1 - t) * coords_a + t * coords_b
        frame = F.grid_sample(image[None], grid[None], mode="bilinear", align_corners=False)[0]
        if certainty is not None:
            white_im = torch.full(certainty.shape, background)
            frame = white_im * (1 - certainty) + certainty * frame
        fl.append(frame.numpy().copy())
        u8.append(np.array(tensor_to_pil(frame, unnormalize=False)))
    return np.stack(fl), np.stack(u8)


def main():
    import morph_cases as cases
    import morph_ref as mr
    ref_import.install_stubs()
    from romatch.utils.utils import tensor_to_pil
    s = cases.build_scene()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items()}
    out = {"in_" + k: v for k, v in s.items()}
    plain = [frames(tensor_to_pil, t["warp"][b], t["image"][b], s["ts"]) for b in range(cases.B)]
    cert = [frames(tensor_to_pil, t["warp"][b], t["image"][b], s["ts_cert"], t["certainty"][b], cases.BACKGROUND) for b in range(cases.B)]
    out["ref_float"], out["ref_u8"] = (np.stack(x) for x in zip(*plain))
    out["ref_cert_float"], out["ref_cert_u8"] = (np.stack(x) for x in zip(*cert))
    assert out["ref_float"].dtype == np.float32 and out["ref_u8"].dtype == np.uint8
    assert out["ref_float"].shape == (cases.B, len(s["ts"]), 3, cases.H, cases.W) and out["ref_u8"].shape == (cases.B, len(s["ts"]), cases.H, cases.W, 3)
    for key in ("", "cert_"):
        fl = np.moveaxis(out[f"ref_{key}float"], -3, -1)
        share = float(mr.excused(fl, cases.U8_MARGIN).mean())
        outside = float((np.abs(s["warp"][..., 2:]) > 1).any(axis=-1).mean())
        print(f"ref_{key}u8: {share * 100:.3f} % of the values excused, {float((fl == 0).mean()) * 100:.1f} % exact zeros; "
              f"{outside * 100:.1f} % of the pixels have a coordinate beyond +-1")
        assert share <= cases.U8_EXCUSED_SHARE
    np.savez_compressed(cases.GOLDEN_FILE, **out)
    size = os.path.getsize(cases.GOLDEN_FILE)
    print(f"{cases.GOLDEN_FILE}: {size} bytes")
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()
