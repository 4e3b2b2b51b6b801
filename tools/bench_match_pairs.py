"""Benchmark of the cached-feature route for image sets (RegressionMatcher.encode_images / match_pairs; csrc/encoded.hip),
after the method of tools/bench_views.py: warm-up, then --rounds rounds in one process, device events around each whole route,
the two routes alternating inside a round; medians and the spread (min / max) over the rounds.

Workload: 8 images, 560 -> 864, mixed precision (bf16 DINOv2, binary16 elsewhere), symmetric, all 28 pairs, max_batch = 8.
  route A   match() on the 28 pairs in batches of 8 (8 + 8 + 8 + 4): every image encoded 7 times
  route B   encode_images(8 images) + match_pairs(all 28 pairs) in the same batches: every image encoded once
B is timed as a whole and as its two halves (an event between them).  The results of the two routes are compared bit for bit
once before the timing.

  python tools/bench_match_pairs.py [--rounds 7] [--out profiles/match_pairs_bench.jsonl]
The share of the gather kernel comes from a separate run under the profiler, which must not time anything itself:
  rocprofv3 --kernel-trace --stats -d DIR -o mp -- python tools/bench_match_pairs.py --profile-run
  python tools/bench_match_pairs.py --stats-csv DIR/.../mp_kernel_stats.csv     (appends the share to the same jsonl)
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IMAGES, COARSE, UPSAMPLE, MAX_BATCH = 8, 560, 864, 8


def setup():
    from roma_amd import roma_model, synthetic
    from roma_amd.encoded import all_pairs
    sd, dsd = synthetic.make_matcher_state_dict(0), synthetic.make_dinov2_state_dict(0)
    d = synthetic.make_inputs(N_IMAGES, COARSE, UPSAMPLE, seed=3)
    x, xh = d["im_A"].cuda(), d["im_A_high_res"].cuda()
    m = roma_model((COARSE, COARSE), True, device="cuda:0", weights=sd, dinov2_weights=dsd, amp_dtype=torch.bfloat16,
                   decoder_dtype=torch.float16, symmetric=True, upsample_res=(UPSAMPLE, UPSAMPLE), max_batch=MAX_BATCH)
    pairs = all_pairs(N_IMAGES)
    ia, ib = [p[0] for p in pairs], [p[1] for p in pairs]
    xa, xb, xha, xhb = x[ia].contiguous(), x[ib].contiguous(), xh[ia].contiguous(), xh[ib].contiguous()  # outside the timed region
    route_a = lambda: m.match(xa, xb, im_A_high_res=xha, im_B_high_res=xhb)  # noqa: E731
    feats = torch.empty(N_IMAGES * m.encoded_bytes(), dtype=torch.uint8, device="cuda:0")
    encode = lambda: m.encode_images(x, xh, out=feats)  # noqa: E731
    return m, pairs, route_a, encode


def stats_share(path, out):
    rows = list(csv.DictReader(open(path)))
    name_k = "Name" if "Name" in rows[0] else "KernelName"
    dur_k = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    total = sum(float(r[dur_k]) for r in rows)
    gather = sum(float(r[dur_k]) for r in rows if "slab_copy" in r[name_k])
    calls = sum(int(float(r["Calls"])) for r in rows if "slab_copy" in r[name_k])
    res = {"call": "route_B_kernel_stats", "gather_kernel": "slab_copy_kernel", "gather_calls": calls,
           "gather_ns": gather, "all_kernels_ns": total, "gather_share": round(gather / total, 5)}
    print(json.dumps(res))
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-run", action="store_true", help="route B three times, nothing timed (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--stats-csv", default=None, help="kernel_stats.csv of such a run: append the gather kernel's share")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_pairs_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.stats_csv:
        return stats_share(args.stats_csv, args.out)
    m, pairs, route_a, encode = setup()
    if args.profile_run:
        for _ in range(3):
            m.match_pairs(encode(), pairs)
        torch.cuda.synchronize()
        return
    wa, ca = route_a()
    wb, cb = m.match_pairs(encode(), pairs)
    torch.cuda.synchronize()
    identical = bool(torch.equal(wa, wb) and torch.equal(ca, cb))
    del wa, ca, wb, cb
    for _ in range(args.warmup):
        route_a()
        m.match_pairs(encode(), pairs)
    torch.cuda.synchronize()
    ms = {"A": [], "B": [], "B_encode": [], "B_match": []}
    for _ in range(args.rounds):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        route_a()
        e[1].record()
        torch.cuda.synchronize()
        e[2].record()
        enc = encode()
        e[3].record()
        m.match_pairs(enc, pairs)
        e[4].record()
        torch.cuda.synchronize()
        ms["A"].append(e[0].elapsed_time(e[1]))
        ms["B_encode"].append(e[2].elapsed_time(e[3]))
        ms["B_match"].append(e[3].elapsed_time(e[4]))
        ms["B"].append(e[2].elapsed_time(e[4]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"call": "match_pairs_vs_match", "images": N_IMAGES, "pairs": len(pairs), "coarse": COARSE, "upsample": UPSAMPLE,
           "precision": "mixed", "max_batch": MAX_BATCH, "rounds": args.rounds, "bit_identical": identical,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(float(min(v)), 3) for k, v in ms.items()},
           "ms_max": {k: round(float(max(v)), 3) for k, v in ms.items()},
           "ratio_A_over_B": round(med["A"] / med["B"], 4),
           "ms_per_pair_A": round(med["A"] / len(pairs), 3), "ms_per_pair_B": round(med["B"] / len(pairs), 3),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
