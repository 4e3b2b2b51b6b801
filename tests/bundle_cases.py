"""What the bundle-adjustment tests share (test_cpu_bundle.py, test_gpu_bundle.py): the scenes of tools/bundle_scenes.py, the
errors of a solution against its scene, and the cut of an oracle run where its decisions stop being decisive."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bundle_ref as br  # noqa: E402
from absolute_pose_cases import f32, rot_angle_deg  # noqa: E402,F401
from bundle_scenes import H, W, scene, start  # noqa: E402,F401


def gauge_error(s, X, R, t, t_start):
    """(|dR|, |dt|, |dX|), largest entries, of a solution under the default hold against the scene: t and X divided by the ratio of
    the held component of t_1 (the start's, which the fit keeps) to the scene's; points with fewer than two observations left out"""
    if len(R) == 1:
        return 0.0, 0.0, 0.0
    c = int(np.argmax(np.abs(t_start[1])))
    ratio = t_start[1, c] / s["t"][1, c]
    seen = np.isfinite(s["kpts"]).all(axis=2).sum(axis=0) >= 2
    return (float(np.abs(R - s["R"]).max()), float(np.abs(t / ratio - s["t"]).max()), float(np.abs(X / ratio - s["X"])[seen].max()))


def pose_errors(s, R, t):
    """median over the views 1 .. V-1 of the rotation error in degrees and of the angle between the translation directions"""
    er = [rot_angle_deg(R[i], s["R"][i]) for i in range(1, len(R))]
    et = [float(np.degrees(np.arccos(np.clip(t[i] @ s["t"][i] / (np.linalg.norm(t[i]) * np.linalg.norm(s["t"][i])), -1, 1)))) for i in range(1, len(R))]
    return float(np.median(er)), float(np.median(et))


def decisive_floor(cost, rows):
    """Device and oracle evaluate the same expressions but add the points in another order, so their states differ by a few ulp
    from the first step on; a residual e then differs by k eps and the cost sum e^2 by up to 2 k eps sum |e| <= 2 k eps
    sqrt(rows cost).  With k = 16: a comparison whose |trial cost - current cost| is below 32 eps sqrt(rows cost) may fall
    either way."""
    return 32 * np.finfo(np.float64).eps * np.sqrt(rows * cost)


def first_undecidable(trace, cost, rows):
    """index of the oracle's first cost comparison that rounding could turn, None when every one is decisive"""
    floor = decisive_floor(cost, rows)
    return next((k for k, (_, _, d) in enumerate(trace) if abs(d) < floor), None)


def decisive_steps(trace, cost, rows):
    """Accepted steps of the oracle's run up to its first cost comparison that rounding could turn (`decisive_floor`): every
    count after it is a property of the rounding, not of the algorithm, and the device is held to the oracle's counts up to
    there."""
    u = first_undecidable(trace, cost, rows)
    return sum(d < 0 for _, _, d in (trace if u is None else trace[:u]))


def oracle_run(s, X0, R0, t0, thr, hold=None):
    """(max_steps, result): the oracle's run of the default 25 steps cut where its decisions stop being decisive, rerun to there"""
    kp = f32(s["kpts"])
    tr = []
    o = br.adjust(X0, kp, s["K"], R0, t0, thr, hold=hold, trace=tr)
    ms = decisive_steps(tr, o["cost"], o["info"][2])
    return ms, br.adjust(X0, kp, s["K"], R0, t0, thr, max_steps=ms, hold=hold)
