"""The reference's demo/demo_3D_effect.py - the parallax animation between two views - with roma_amd: match once, then render all
frames in ONE roma_amd.render_morph call (the reference runs a lerp, a grid_sample and a device-to-host copy per frame), and write
them through Pillow on the host.  An example; no test depends on it.

    python tools/demo_3d_effect.py --im_A_path A.jpg --im_B_path B.jpg --weights roma_outdoor.pth --dinov2_weights dinov2_vitl14.pth
    python tools/demo_3d_effect.py --synthetic --gif morph.gif          # a seeded smooth warp over a generated picture: no weights

Frames go to <save_path>_000.jpg ... as in the reference, or into one GIF with --gif."""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def synthetic(H, W, seed=0):
    """(warp f32 [H, W, 4], picture uint8 [H, W, 3]) on the device: the pixel centres, a smooth parallax-like displacement of them,
    and a picture of coloured rings and bars in which the displacement is easy to see"""
    rng = np.random.default_rng(seed)
    ys, xs = (2.0 * np.arange(H) + 1.0) / H - 1.0, (2.0 * np.arange(W) + 1.0) / W - 1.0
    y, x = np.meshgrid(ys, xs, indexing="ij")
    p = rng.random(4) * 6.0
    depth = 0.5 + 0.5 * np.exp(-((x - 0.2) ** 2 + (y + 0.1) ** 2) / 0.18)  # a bump that is nearer than its surroundings
    bx = x + 0.12 * depth + 0.02 * np.sin(2.0 * y + p[0])
    by = y + 0.03 * depth * np.cos(1.5 * x + p[1])
    warp = np.stack([x, y, bx, by], axis=-1).astype(np.float32)
    r = np.sqrt((x - 0.2) ** 2 + (y + 0.1) ** 2)
    pic = np.stack([0.5 + 0.5 * np.sin(40.0 * r + p[2]), 0.5 + 0.5 * np.sin(25.0 * x + p[3]), 0.5 + 0.5 * np.cos(25.0 * y)], axis=-1)
    return torch.from_numpy(warp).to(DEV), torch.from_numpy((pic * 255).astype(np.uint8)).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--im_A_path", default="assets/toronto_A.jpg")
    ap.add_argument("--im_B_path", default="assets/toronto_B.jpg")
    ap.add_argument("--save_path", default="roma_warp")
    ap.add_argument("--gif", default=None, help="write one GIF here instead of a JPEG per frame")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--res", type=int, nargs=2, default=[864, 1152], help="H W of the frames (the matcher's upsample_res)")
    ap.add_argument("--synthetic", action="store_true", help="a seeded smooth warp over a generated picture; needs no weights")
    ap.add_argument("--weights", default=None, help="roma_outdoor state dict (.pth)")
    ap.add_argument("--dinov2_weights", default=None, help="DINOv2 ViT-L/14 state dict (.pth)")
    ap.add_argument("--certainty", action="store_true", help="blend the frames over white by the matcher's certainty")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "demo_3d_effect.py renders on the device: it needs a GPU"
    import roma_amd
    H, W = args.res
    certainty = None
    if args.synthetic:
        warp, picture = synthetic(H, W)
    else:
        if not (args.weights and args.dinov2_weights):
            ap.error("--weights and --dinov2_weights are required without --synthetic")
        model = roma_amd.roma_outdoor(DEV, weights=torch.load(args.weights, map_location="cpu"),
                                      dinov2_weights=torch.load(args.dinov2_weights, map_location="cpu"), coarse_res=560,
                                      upsample_res=(H, W), symmetric=False)
        warp, cert = model.match(args.im_A_path, args.im_B_path, device=DEV)
        certainty = cert if args.certainty else None
        picture = torch.from_numpy(np.array(Image.open(args.im_B_path).convert("RGB").resize((W, H)))).to(DEV)  # uint8 [H, W, 3]
    frames = roma_amd.render_morph(warp, picture, roma_amd.morph_times(args.frames), certainty=certainty)  # uint8 [T, H, W, 3]
    frames = frames.cpu().numpy()  # the one device-to-host copy
    if args.gif:
        ims = [Image.fromarray(f) for f in frames]
        ims[0].save(args.gif, save_all=True, append_images=ims[1:], duration=40, loop=0)
        print(f"{args.gif}: {len(ims)} frames of {W} x {H}")
    else:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_path)), exist_ok=True)
        for i, f in enumerate(frames):
            Image.fromarray(f).save(f"{args.save_path}_{i:03d}.jpg")
        print(f"{args.save_path}_000.jpg ... _{len(frames) - 1:03d}.jpg: {W} x {H}")


if __name__ == "__main__":
    main()
