"""Per-step figures of the two latency-bound chains from a rocprofv3 --kernel-trace CSV of bench.py:
 (a) the local-correlation sort stage: every kernel a queue runs between the tile kernel that follows a classifier and the LIST
     tile kernel (memset kernels included), per radius;
 (b) the chol_col_kernel launches per block column (chains of 25 launches per queue: n = 1600).
Both sub-batch streams run at once in the traced step, so a kernel's duration includes what its neighbour on the other queue
costs it: mean, median and minimum are printed.
usage: latency_chains_trace.py <kernel_trace.csv> <steps in the trace, warm-up included> <label>"""
import csv
import re
import statistics
import sys
from collections import defaultdict

NBLK = 25


def main():
    path, nsteps, label = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    ev = defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            ev[int(r["Queue_Id"])].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    stage = defaultdict(list)                          # radius -> kernel time of the stage, per call (us)
    parts = defaultdict(lambda: defaultdict(list))     # radius -> kernel -> durations (us)
    classify = defaultdict(list)                       # radius -> durations of the classifier in front of the stage (us)
    chol = defaultdict(list)
    nchains = 0
    for lst in ev.values():
        lst.sort()
        i = 0
        while i < len(lst):
            m = re.search(r"local_corr_classify_kernel<\(?(?:int\))?(\d+)", lst[i][2])
            if not m:
                i += 1
                continue
            classify[int(m.group(1))].append((lst[i][1] - lst[i][0]) / 1e3)
            j, tiles_seen, inside = i + 1, 0, []
            while j < len(lst) and tiles_seen < 2:
                if "local_corr_tile_kernel" in lst[j][2]:
                    tiles_seen += 1
                elif "local_corr_list_kernel" in lst[j][2]:
                    tiles_seen = 99
                elif tiles_seen == 1:
                    inside.append(lst[j])
                j += 1
            if tiles_seen == 2 and inside:
                R = int(m.group(1))
                stage[R].append(sum(e - b for b, e, _ in inside) / 1e3)
                per = defaultdict(float)
                for b, e, n in inside:
                    per[re.sub(r"\(.*", "", n).replace("void ", "")] += (e - b) / 1e3
                for n, d in per.items():
                    parts[R][n].append(d)
            i = j
        cc = [(b, e) for b, e, n in lst if "chol_col_kernel" in n]
        for c0 in range(0, len(cc) - NBLK + 1, NBLK):
            nchains += 1
            for k in range(NBLK):
                chol[k].append((cc[c0 + k][1] - cc[c0 + k][0]) / 1e3)

    print(f"== {label}: {nsteps} steps in the trace (warm-up included)")
    print("-- (a) sort stage between the tile kernel and the LIST tile kernel: kernel time, us")
    tot = tot_med = 0.0
    for R in sorted(stage):
        v = stage[R]
        print(f"r={R}: {len(v) / nsteps:.0f} calls/step; per call mean {statistics.mean(v):6.1f} median {statistics.median(v):6.1f} min {min(v):6.1f}; "
              f"per step {sum(v) / nsteps:7.1f}")
        for n, d in sorted(parts[R].items(), key=lambda x: -sum(x[1])):
            print(f"      mean {statistics.mean(d):6.1f} median {statistics.median(d):6.1f} min {min(d):6.1f}  {n}")
        tot += sum(v) / nsteps
        tot_med += statistics.median(v) * len(v) / nsteps
    print(f"all radii, per step: {tot:.1f} us (sum of all calls / steps); {tot_med:.1f} us with every call at its radius' median")
    print("-- the classifier in front of the stage (outside the figure above), us per call")
    for R in sorted(classify):
        v = classify[R]
        print(f"r={R}: mean {statistics.mean(v):6.1f} median {statistics.median(v):6.1f} min {min(v):6.1f}; per step {sum(v) / nsteps:7.1f}")
    print(f"all radii, per step: {sum(sum(v) for v in classify.values()) / nsteps:.1f} us")
    if len(chol) == NBLK:
        print(f"-- (b) chol_col_kernel per column, us, over {nchains} chains ({nchains / nsteps:.0f} per step)")
        for k in range(NBLK):
            print(f"k={k:2d} mean {statistics.mean(chol[k]):6.1f} median {statistics.median(chol[k]):6.1f} min {min(chol[k]):6.1f}")
        for name, fn in (("mean", statistics.mean), ("median", statistics.median), ("min", min)):
            ys = [fn(chol[k]) for k in range(NBLK)]
            ks = list(range(2, NBLK))
            mk, my = statistics.mean(ks), statistics.mean(ys[2:])
            slope = sum((k - mk) * (ys[k] - my) for k in ks) / sum((k - mk) ** 2 for k in ks)
            print(f"chain sum of the columns' {name}: {sum(ys):7.1f} us; slope over k = 2..{NBLK - 1}: {slope:.3f} us per column, "
                  f"sum over k >= 2 of (k - 1) x slope = {slope * sum(k - 1 for k in ks):.1f} us")


if __name__ == "__main__":
    main()
