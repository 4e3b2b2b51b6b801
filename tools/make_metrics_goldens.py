"""Build-container only: record what the UNMODIFIED reference makes of the cases of tests/metrics_cases.py in
tests/golden/metrics_reference.npz - inputs (in_*), checksums of generated inputs (chk_*) and recorded outputs (ref_*) only, no
reference program text.

    python tools/make_metrics_goldens.py

romatch/utils/utils.py compute_pose_error on the first GOLDEN_POSE_ROWS pose rows with ok == 1 (the rows with ok == 0 never reach
it: the benchmarks' except branch scores them 90) and pose_auc on every error set, at the pose benchmarks' thresholds (5, 10, 20)
and the HPatches benchmark's (1 .. 10).  The HPatches corner distance is inline in the reference's benchmark loop and cannot be
called, so it has no recorded output."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402


def main():
    import metrics_cases as cases
    ref_import.install_stubs()
    import romatch.utils.utils as U
    if not hasattr(np, "trapz"):  # numpy 2.4 dropped the old name of the same function
        np.trapz = np.trapezoid
    p = cases.pose_cases()
    n = cases.GOLDEN_POSE_ROWS
    out = {"in_" + k: np.array(p[k][:n]) for k in ("R", "t", "T", "ok")}
    e_t, e_R = np.full(n, np.nan), np.full(n, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the zero translation divides 0 by 0
        for b in range(n):
            if p["ok"][b]:
                e_t[b], e_R[b] = U.compute_pose_error(p["T"][b], p["R"][b], p["t"][b])
    out["ref_e_t"], out["ref_e_R"] = e_t, e_R
    for name, e in cases.error_sets().items():
        out["chk_" + name] = np.array(cases.checksum(e), dtype=np.uint64)
        out["ref_auc_pose_" + name] = np.array(U.pose_auc(np.array(e), list(cases.REFERENCE_POSE_THRESHOLDS)), dtype=np.float64)
        out["ref_auc_homog_" + name] = np.array(U.pose_auc(np.array(e), [int(t) for t in cases.HOMOGRAPHY_THRESHOLDS]), dtype=np.float64)
    np.savez_compressed(cases.GOLDEN_FILE, **out)
    size = os.path.getsize(cases.GOLDEN_FILE)
    print(f"{cases.GOLDEN_FILE}: {size} bytes; {int(p['ok'][:n].sum())} of {n} pose rows scored, {len(cases.error_sets())} error sets")
    for name in cases.error_sets():
        print(f"  {name}: pose_auc {out['ref_auc_pose_' + name]}")
    assert size < 32 * 1024


if __name__ == "__main__":
    main()
