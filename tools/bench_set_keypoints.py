"""Microbenchmark of the detector-free keypoints (roma_amd.keypoints_from_matches; csrc/set_keypoints.hip), after the method of
tools/bench_views.py: the calls are timed alternately in --rounds rounds of --iters calls each, device events around each block
after a warm-up of every call, medians over the rounds.

  keypoints_from_matches   8 views at 864 x 1152, all 28 pairs, 5 000 rows each, cell 2, B in {1, 8}: 5 000 scene points per
                           problem seen in every view, +-0.25 px of jitter per endpoint, certainties from {1, 0.5, 0.2}
  torch yardstick          the same device, without suppression, assignment or one-to-one: pixel conversion, floor,
                           torch.unique over the cell ids of a view and scatter_reduce(amax) of the certainties, view by view
  stages                   the time of each of the seven kernels, from the library's per-launch events in a pass of its own

One JSON line per call appended to profiles/set_keypoints_bench.jsonl, the per-kernel figures to
profiles/set_keypoints_bench_kernel_stats.csv.
Usage: python tools/bench_set_keypoints.py [--iters 20] [--rounds 9] [--out profiles/set_keypoints_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, H, W, N, CELL = 8, 864, 1152, 5000, 2
PAIRS = [(a, b) for a in range(V) for b in range(a + 1, V)]


def problem(seed):
    """(matches [P, N, 4] normalised f32, certainty [P, N] f32): N scene points with a position in every view"""
    g = np.random.default_rng(seed)
    where = np.stack([g.uniform(1, W - 1, (V, N)), g.uniform(1, H - 1, (V, N))], axis=-1)
    m = np.zeros((len(PAIRS), N, 4), np.float32)
    for p, (a, b) in enumerate(PAIRS):
        for side, v in enumerate((a, b)):
            px = where[v] + g.uniform(-0.25, 0.25, (N, 2))
            m[p, :, 2 * side], m[p, :, 2 * side + 1] = 2 * px[:, 0] / W - 1, 2 * px[:, 1] / H - 1
    return m, g.choice(np.array([1.0, 0.5, 0.2], np.float32), (len(PAIRS), N))


def torch_route(m, c, view_rows):
    """per problem and view: the occupied cells and their best certainty - no suppression, no assignment, no one-to-one"""
    out = []
    Gw = (W + CELL - 1) // CELL
    for b in range(m.shape[0]):
        for v in range(V):
            p, side = view_rows[v]
            xy = torch.cat([m[b, p[side == 0], :, 0:2].reshape(-1, 2), m[b, p[side == 1], :, 2:4].reshape(-1, 2)])
            cc = torch.cat([c[b, p[side == 0]].reshape(-1), c[b, p[side == 1]].reshape(-1)])
            x, y = (W * 0.5) * (xy[:, 0] + 1), (H * 0.5) * (xy[:, 1] + 1)
            cell = (torch.floor(y).long() // CELL) * Gw + torch.floor(x).long() // CELL
            ids, inv = torch.unique(cell, return_inverse=True)
            out.append((ids, torch.zeros(ids.shape[0], device=m.device).scatter_reduce(0, inv, cc, "amax")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_keypoints_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_set_keypoints: no HIP device (there is no CPU fallback and no CPU timing)")
    from roma_amd import _lib, keypoints_from_matches
    dev = "cuda:0"
    sizes = [(H, W)] * V
    view_rows = []
    for v in range(V):
        rows = [(p, s) for p, pr in enumerate(PAIRS) for s in range(2) if pr[s] == v]
        view_rows.append((torch.tensor([p for p, _ in rows], device=dev), torch.tensor([s for _, s in rows], device=dev)))
    calls, extra = {}, {}
    for B in (1, 8):
        ms_, cs_ = zip(*(problem(b) for b in range(B)))
        m, c = torch.tensor(np.stack(ms_), device=dev), torch.tensor(np.stack(cs_), device=dev)
        calls[f"keypoints_from_matches B={B}"] = lambda m=m, c=c: keypoints_from_matches(m, c, PAIRS, V, sizes, cell=CELL)
        calls[f"keypoints_from_matches B={B} radius=0 one_to_one=False"] = lambda m=m, c=c: keypoints_from_matches(m, c, PAIRS, V, sizes, cell=CELL, radius=0.0,
                                                                                                                  one_to_one=False)
        calls[f"torch unique + scatter_reduce B={B}"] = lambda m=m, c=c: torch_route(m, c, view_rows)
        extra[f"keypoints_from_matches B={B}"] = lambda out, B=B: {"B": B, "V": V, "P": len(PAIRS), "N": N, "cell": CELL, "size": [H, W],
                                                                   "num_kpts": out.num_kpts.reshape(-1, V)[0].cpu().tolist(),
                                                                   "info": out.info.reshape(-1, 6)[0].cpu().tolist()}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the yardstick finds the same cells as the operator with suppression off
    off, ref = calls["keypoints_from_matches B=1 radius=0 one_to_one=False"](), calls["torch unique + scatter_reduce B=1"]()
    if off.num_kpts[0].cpu().tolist() != [len(ids) for ids, _ in ref] or not all(
            torch.equal(off.score[0, v, :len(s)], s) for v, (_, s) in enumerate(ref)):
        raise SystemExit("bench_set_keypoints: the torch yardstick does not find the operator's cells")
    ms = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.iters)
    # the kernels, in a pass of their own
    lib = _lib.load()
    stages = {}
    for B in (1, 8):
        lib.roma_profile_enable(1)
        for _ in range(args.iters):
            calls[f"keypoints_from_matches B={B}"]()
        torch.cuda.synchronize()
        n = lib.roma_profile_report(None, 0)
        buf = C.create_string_buffer(int(n))
        lib.roma_profile_report(buf, n)
        lib.roma_profile_enable(0)
        stages[B] = {k: round(v["total_ms"] / v["calls"], 4) for k, v in json.loads(buf.value.decode()).items() if k.startswith("skp_")}
    lines = []
    for name in ms:
        res = {"call": name, "iters": args.iters, "rounds": args.rounds, "ms_per_call_median": round(float(np.median(ms[name])), 4),
               "ms_per_call_min": round(float(np.min(ms[name])), 4), "ms_per_call_max": round(float(np.max(ms[name])), 4),
               "device": torch.cuda.get_device_name(0)}
        if name in extra:
            res.update(extra[name](calls[name]()))
            res["stage_ms"] = stages[res["B"]]
            res["torch_yardstick_over_this"] = round(float(np.median(ms[f"torch unique + scatter_reduce B={res['B']}"]) / np.median(ms[name])), 2)
        print(json.dumps(res), flush=True)
        lines.append(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")
    with open(os.path.splitext(args.out)[0] + "_kernel_stats.csv", "w") as f:
        f.write("B,kernel,ms_per_call\n")
        for B, st in stages.items():
            for k, v in st.items():
                f.write(f"{B},{k},{v}\n")


if __name__ == "__main__":
    main()
