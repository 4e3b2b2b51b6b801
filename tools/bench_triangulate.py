"""Microbenchmark of the on-device triangulation (roma_amd.triangulate / triangulate_warp, csrc/triangulate.hip) against what a
user writes today, the same formulas as torch elementwise passes in float64 on the same device:
  dense   B = 8 symmetric warps of 864 x 2304 points (H = 864, W = 1152), with and without the depth-consistency pass;
  sparse  B = 8 x 5 000 sampled matches in pixels.
Both legs run in one process on the same tensors, timed alternately (A B A B) with device events after a warm-up: --rounds rounds
of --iters calls per leg, medians and spread over the rounds.  Besides ms per call the line holds the algorithmic bytes over the
time (20 B read and 25 B written per point; the consistency pass 13 B + 1 B), next to the 6.29 TB/s a float4 copy reaches on an
MI355X.  One JSON line per configuration, appended to --out (profiles/triangulate_bench.jsonl) and printed.
Usage: python tools/bench_triangulate.py [--iters 10] [--rounds 5] [--only hip|torch] [--config dense dense_consistency sparse]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
COPY_RATE = 6.29e12  # B/s, float4 copy on an MI355X
SIZES = (640, 480, 512, 360)  # W_a, H_a, W_b, H_b
K_A = torch.tensor([[520.0, 0.0, 325.0], [0.0, 510.0, 236.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
K_B = torch.tensor([[430.0, 0.0, 250.0], [0.0, 425.0, 185.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
THRESHOLDS = dict(max_depth=30.0, max_reproj=1.5, min_parallax=0.5, min_certainty=0.25)


def poses(B):
    """B small rotations about (nearly) the y axis and sideways translations, float64 on the device"""
    ang = -(0.08 + 0.01 * torch.arange(B, dtype=torch.float64))
    R = torch.zeros(B, 3, 3, dtype=torch.float64)
    R[:, 0, 0], R[:, 0, 2], R[:, 2, 0], R[:, 2, 2], R[:, 1, 1] = torch.cos(ang), torch.sin(ang), -torch.sin(ang), torch.cos(ang), 1.0
    t = torch.stack((0.5 + 0.02 * torch.arange(B, dtype=torch.float64), torch.full((B,), 0.03, dtype=torch.float64),
                     torch.full((B,), 0.08, dtype=torch.float64)), dim=-1)
    return R.to(DEV), t.to(DEV)


def plane_warp(B, H, W, R, t, noise_px=0.3, seed=0):
    """symmetric warps [B, H, 2W, 4] of the plane n . X = 4 under the poses, with pixel noise on the predicted side, and a
    uniform certainty [B, H, 2W]"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    Wa, Ha, Wb, Hb = SIZES
    ka, kb = K_A.to(DEV), K_B.to(DEV)
    nrm = torch.tensor([0.15, -0.10, 1.0], dtype=torch.float64, device=DEV)
    nrm = nrm / nrm.norm()
    gx = ((torch.arange(W, device=DEV, dtype=torch.float64) + 0.5) / W * 2 - 1)[None, None, :].expand(B, H, W)
    gy = ((torch.arange(H, device=DEV, dtype=torch.float64) + 0.5) / H * 2 - 1)[None, :, None].expand(B, H, W)

    def rays(k, w, h):
        return torch.stack((((gx + 1) * w / 2 - k[0, 2]) / k[0, 0], ((gy + 1) * h / 2 - k[1, 2]) / k[1, 1], torch.ones_like(gx)), -1)

    def norm_proj(k, X, w, h):
        p = torch.stack((k[0, 0] * X[..., 0] / X[..., 2] + k[0, 2], k[1, 1] * X[..., 1] / X[..., 2] + k[1, 2]), -1)
        p = p + noise_px * torch.randn(p.shape, device=DEV, dtype=torch.float64, generator=g)
        return torch.stack((2 * p[..., 0] / w - 1, 2 * p[..., 1] / h - 1), -1)
    xa = rays(ka, Wa, Ha)
    Xa = xa * (4.0 / (xa @ nrm))[..., None]
    left = torch.cat((torch.stack((gx, gy), -1), norm_proj(kb, torch.einsum("bij,bhwj->bhwi", R, Xa) + t[:, None, None], Wb, Hb)), -1)
    nb = torch.einsum("bij,j->bi", R, nrm)
    cb = 4.0 + (nb * t).sum(-1)
    xb = rays(kb, Wb, Hb)
    Xb = xb * (cb[:, None, None] / torch.einsum("bhwj,bj->bhw", xb, nb))[..., None]
    right = torch.cat((norm_proj(ka, torch.einsum("bji,bhwj->bhwi", R, Xb - t[:, None, None]), Wa, Ha), torch.stack((gx, gy), -1)), -1)
    warp = torch.cat((left, right), dim=2).float().contiguous()
    cert = torch.rand((B, H, 2 * W), device=DEV, generator=g)
    return warp, cert


# --------------------------------------------------------------------------------------------- the torch restatement
def torch_view(ref, obs, cert, R, t, kr, ko, th):
    """tools/triangulate_ref.triangulate_view in torch: ref, obs [B, m, 2] float64 pixels, R [B, 3, 3], t [B, 3], k (fx, fy, cx, cy)"""
    u, v, uo, vo = ref[..., 0], ref[..., 1], obs[..., 0], obs[..., 1]
    r = lambda i, j: R[:, i, j, None]  # noqa: E731
    t0, t1, t2 = t[:, 0, None], t[:, 1, None], t[:, 2, None]
    x0, x1 = (u - kr[2]) / kr[0], (v - kr[3]) / kr[1]
    r0, r1, r2 = (r(0, 0) * x0 + r(0, 1) * x1) + r(0, 2), (r(1, 0) * x0 + r(1, 1) * x1) + r(1, 2), (r(2, 0) * x0 + r(2, 1) * x1) + r(2, 2)
    A0, A1, A2 = ko[0] * r0 + ko[2] * r2, ko[1] * r1 + ko[3] * r2, r2
    bv0, bv1, bv2 = ko[0] * t0 + ko[2] * t2, ko[1] * t1 + ko[3] * t2, t2
    l0, l1, l2 = A1 * bv2 - A2 * bv1, A2 * bv0 - A0 * bv2, A0 * bv1 - A1 * bv0
    n2 = l0 * l0 + l1 * l1
    degenerate = ~(torch.isfinite(u) & torch.isfinite(v) & torch.isfinite(uo) & torch.isfinite(vo) & (n2 > 0))
    s = (l0 * uo + l1 * vo) + l2
    d = s / torch.sqrt(n2)
    px, py = uo - (s * l0) / n2, vo - (s * l1) / n2
    a0, a1 = px * A2 - A0, py * A2 - A1
    b0, b1 = bv0 - px * bv2, bv1 - py * bv2
    z = (a0 * b0 + a1 * b1) / (a0 * a0 + a1 * a1)
    zo = z * r2 + t2
    h0, h1 = (px - ko[2]) / ko[0], (py - ko[3]) / ko[1]
    c0, c1, c2 = r1 - r2 * h1, r2 * h0 - r0, r0 * h1 - r1 * h0
    par = torch.atan2(torch.sqrt((c0 * c0 + c1 * c1) + c2 * c2), (r0 * h0 + r1 * h1) + r2) * 57.29577951308232
    flags = (~((z > 0) & (z < th["max_depth"])) | ~((zo > 0) & (zo < th["max_depth"]))).to(torch.uint8) * 4
    flags = flags + (~(d.abs() <= th["max_reproj"])).to(torch.uint8) * 8 + (~(par >= th["min_parallax"])).to(torch.uint8) * 16
    if cert is not None:
        flags = flags + (~(cert >= th["min_certainty"])).to(torch.uint8) * 32
    flags = torch.where(degenerate, torch.full_like(flags, 2), flags)
    nan = torch.full_like(z, float("nan"))
    pts = torch.stack((torch.where(degenerate, nan, z * x0), torch.where(degenerate, nan, z * x1), torch.where(degenerate, nan, z)), -1)
    return pts.float(), torch.where(degenerate, nan, zo).float(), torch.where(degenerate, nan, d).float(), torch.where(degenerate, nan, par).float(), flags


def cam(K):
    return (K[0, 0].item(), K[1, 1].item(), K[0, 2].item(), K[1, 2].item())


def to_pix(x, w, h):
    x = x.double()
    return torch.stack(((x[..., 0] + 1) * w / 2, (x[..., 1] + 1) * h / 2), -1)


def torch_warp(warp, cert, R, t, th, W):
    """both halves of a symmetric warp [B, H, 2W, 4]: five [B, H, 2W(, 3)] outputs"""
    Wa, Ha, Wb, Hb = SIZES
    B, H = warp.shape[0], warp.shape[1]
    Ri = R.transpose(1, 2)
    ti = -torch.einsum("bij,bj->bi", Ri, t)
    lw, rw = warp[:, :, :W].reshape(B, -1, 4), warp[:, :, W:].reshape(B, -1, 4)
    a = torch_view(to_pix(lw[..., 0:2], Wa, Ha), to_pix(lw[..., 2:4], Wb, Hb), cert[:, :, :W].reshape(B, -1), R, t, cam(K_A), cam(K_B), th)
    b = torch_view(to_pix(rw[..., 2:4], Wb, Hb), to_pix(rw[..., 0:2], Wa, Ha), cert[:, :, W:].reshape(B, -1), Ri, ti, cam(K_B), cam(K_A), th)
    return tuple(torch.cat((x.reshape((B, H, W) + x.shape[2:]), y.reshape((B, H, W) + y.shape[2:])), dim=2) for x, y in zip(a, b))


def torch_consistency(points, flags, R, t, W, rel=0.05):
    """tools/triangulate_ref.depth_consistency in torch on [B, H, 2W, 3] points and [B, H, 2W] flags"""
    Wa, Ha, Wb, Hb = SIZES
    B, H = points.shape[0], points.shape[1]
    Z, ok = points[..., 2].double(), flags == 0
    out = []
    for half in (0, 1):
        X = points[:, :, half * W:(half + 1) * W].double()
        if half == 0:
            Y = torch.einsum("bij,bhwj->bhwi", R, X) + t[:, None, None]
            k, wo, ho, off = cam(K_B), Wb, Hb, W
        else:
            Y = torch.einsum("bji,bhwj->bhwi", R, X - t[:, None, None])
            k, wo, ho, off = cam(K_A), Wa, Ha, 0
        gx = (k[0] * (Y[..., 0] / Y[..., 2]) + k[2]) / wo * W - 0.5
        gy = (k[1] * (Y[..., 1] / Y[..., 2]) + k[3]) / ho * H - 0.5
        fx0, fy0 = torch.floor(gx), torch.floor(gy)
        inside = ok[:, :, half * W:(half + 1) * W] & (fx0 >= 0) & (fx0 + 1 <= W - 1) & (fy0 >= 0) & (fy0 + 1 <= H - 1)
        xi = torch.where(inside, fx0, torch.zeros_like(fx0)).long() + off
        yi = torch.where(inside, fy0, torch.zeros_like(fy0)).long()
        lin = (yi * (2 * W) + xi).reshape(B, -1)
        take = lambda src, o: torch.gather(src.reshape(B, -1), 1, (lin + o).clamp(max=H * 2 * W - 1)).reshape(B, H, W)  # noqa: E731
        sup = inside & take(ok, 0) & take(ok, 1) & take(ok, 2 * W) & take(ok, 2 * W + 1)
        ax, ay = gx - fx0, gy - fy0
        v = (take(Z, 0) * (1 - ax) + take(Z, 1) * ax) * (1 - ay) + (take(Z, 2 * W) * (1 - ax) + take(Z, 2 * W + 1) * ax) * ay
        e = (v - Y[..., 2]).abs() / v
        out.append(torch.where(sup, (e < rel).to(torch.uint8), torch.full_like(flags[:, :, :W], 2)))
    return torch.cat(out, dim=2)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=864)
    ap.add_argument("--width", type=int, default=1152)
    ap.add_argument("--num", type=int, default=5000)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--config", nargs="+", default=["dense", "dense_consistency", "sparse"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_triangulate.py measures the device path: it needs a GPU"
    import roma_amd
    B, H, W = args.batch, args.height, args.width
    R, t = poses(B)
    warp, cert = plane_warp(B, H, W, R, t)
    Wa, Ha, Wb, Hb = SIZES
    ka, kb = K_A.to(DEV), K_B.to(DEV)
    idx = torch.randint(0, H * W, (B, args.num), device=DEV)
    left = warp[:, :, :W].reshape(B, -1, 4)
    sm = torch.gather(left, 1, idx[..., None].expand(B, args.num, 4))
    sparse = torch.cat((to_pix(sm[..., 0:2], Wa, Ha), to_pix(sm[..., 2:4], Wb, Hb)), -1).float().contiguous()
    scert = torch.gather(cert[:, :, :W].reshape(B, -1), 1, idx).contiguous()
    n_dense = B * H * 2 * W
    configs = {
        "dense": (45 * n_dense, lambda: roma_amd.triangulate_warp(warp, cert, R, t, ka, kb, Ha, Wa, Hb, Wb, symmetric=True, **THRESHOLDS),
                  lambda: torch_warp(warp, cert, R, t, THRESHOLDS, W)),
        "dense_consistency": ((45 + 14) * n_dense,
                              lambda: roma_amd.triangulate_warp(warp, cert, R, t, ka, kb, Ha, Wa, Hb, Wb, symmetric=True, consistency=True, **THRESHOLDS),
                              lambda: (lambda o: torch_consistency(o[0], o[4], R, t, W))(torch_warp(warp, cert, R, t, THRESHOLDS, W))),
        "sparse": (45 * B * args.num, lambda: roma_amd.triangulate(sparse, None, R, t, ka, kb, certainty=scert, **THRESHOLDS),
                   lambda: torch_view(sparse[..., 0:2].double(), sparse[..., 2:4].double(), scert, R, t, cam(K_A), cam(K_B), THRESHOLDS)),
    }
    for name in args.config:
        nbytes, hip, ref = configs[name]
        legs = {"hip ms": hip, "torch ms": ref}
        if args.only:
            legs = {k: v for k, v in legs.items() if k.startswith(args.only)}
        for fn in legs.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k].append(timed(fn, args.iters))
        res = {"config": f"triangulate {name}", "B": B, "points": n_dense if name != "sparse" else B * args.num,
               "grid": [H, 2 * W] if name != "sparse" else None, "rounds": args.rounds, "iters_per_round": args.iters,
               "algorithmic bytes": nbytes, **{k: stats(v) for k, v in ms.items()}}
        if "hip ms" in ms:
            rate = nbytes / (np.median(ms["hip ms"]) * 1e-3)
            res["hip TB/s"] = round(rate / 1e12, 3)
            res["share of the 6.29 TB/s copy rate"] = round(rate / COPY_RATE, 3)
        if len(legs) == 2:
            res["torch over hip"] = round(float(np.median(ms["torch ms"]) / np.median(ms["hip ms"])), 2)
            res["hip faster than torch in every round"] = bool(np.max(ms["hip ms"]) < np.min(ms["torch ms"]))
            if name == "dense":  # the two legs compute the same thing
                o, r = hip(), ref()
                res["flags equal"] = round(float((torch.cat((o.flags_A, o.flags_B), 2) == r[4]).float().mean()), 6)
                res["valid share"] = round(float((r[4] == 0).float().mean()), 4)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
