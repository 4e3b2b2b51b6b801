"""numpy float64 restatement of the device Levenberg-Marquardt loop (roma_amd/csrc/lm_fit.h `lm_fit`): the part that
tools/pose_refine_ref.py and tools/model_refine_ref.py, the oracles of the refinement kernels, have in common - as the kernels
have the header in common.  A problem hands `fit` its residuals, Jacobian, normal equations and update; the constants, the truncated
cost, the damped Cholesky solve and the order of decisions are here.

  cost        sum of |r|^2 over the active rows (|r|^2 < thr^2) + thr^2 (n - active); a non-finite residual is never active;
              thr = inf is plain least squares over the finite rows (the second term is then dropped)
  iteration   H = J^T J, g = J^T r over the active rows; (H + lambda diag H) delta = -g by Cholesky (`solve`: not positive
              definite when a pivot is not above PIVOT_REL times the largest diagonal entry); |delta| < STEP_TOL stops; the
              trial is accepted when its cost is strictly lower (lambda <- max(lambda / 10, LAMBDA_MIN)), else lambda <- 10 lambda
              and the solve is repeated, at most RETRIES times
  stop        max_steps accepted steps, a short step, RETRIES failed retries, fewer than min_rows active rows (H = J^T J of
              fewer rows than parameters is singular; an empty active set is the common case of a start outside the threshold
              band), not positive definite: the state so far is returned, so the truncated cost never rises
"""
from __future__ import annotations

import math

import numpy as np

LAMBDA0 = 1e-3
LAMBDA_MIN = 1e-10
RETRIES = 10          # retries of one step with a ten times larger lambda
STEP_TOL = 1e-10      # |delta| below which the fit has converged
PIVOT_REL = 1e-14     # Cholesky pivot / largest diagonal entry of H + lambda diag H


def active(e, thr):
    """(active rows, |e|^2 per row) of the residuals e [n, NR]"""
    with np.errstate(all="ignore"):
        r2 = (e * e).sum(axis=1) if e.shape[1] == 1 else e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        return np.isfinite(r2) & (r2 < thr * thr), r2


def truncated(e, thr):
    """(truncated cost, active rows [n]); with thr^2 = inf (plain least squares) the rows that are not active - the non-finite
    ones - are the same for every model and cost nothing"""
    a, r2 = active(e, thr)
    thr2 = thr * thr
    return float(r2[a].sum() + (thr2 * (len(r2) - int(a.sum())) if math.isfinite(thr2) else 0.0)), a


def solve(H, g, lam):
    """delta of (H + lam diag H) delta = -g by Cholesky, or None when a pivot is not above PIVOT_REL x the largest diagonal"""
    n = len(g)
    A = np.array(H, dtype=np.float64)
    A[np.arange(n), np.arange(n)] = np.diag(H) + lam * np.diag(H)
    big = A.diagonal().max()
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not d > PIVOT_REL * big:
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            s = A[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        s = -g[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s / L[i, i]
    d = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s = s - L[k, i] * d[k]
        d[i] = s / L[i, i]
    return d


def fit(P, st, w, thr, max_steps):
    """The loop from the state `st` of the problem P on the rows w - the policy of the device's lm_fit<P>: P.MIN_ROWS,
    P.jacobian(st, w) -> (e [n, NR], J), P.normal(J, e, a) -> (H = J^T J, g = J^T e over the active rows a), P.residuals(st, w)
    -> e [n, NR], P.apply(st, delta) -> the state after the step.  The product is the problem's because numpy forms A.T @ A of
    one buffer by syrk and of two copies by gemm, which differ in the last bits: each oracle keeps the form it had when the
    device tolerances of its tests were measured against it.  Returns (final state, accepted steps, cost evaluations, active
    rows [n] at the end, truncated cost at the start, at the end)."""
    lam, steps, evals = LAMBDA0, 0, 1
    e, J = P.jacobian(st, w)
    cur, a = truncated(e, thr)
    cost0 = cur
    while steps < max_steps and int(a.sum()) >= P.MIN_ROWS:
        H, g = P.normal(J, e, a)
        taken = stop = False
        for _ in range(1 + RETRIES):
            d = solve(H, g, lam)
            if d is None or math.sqrt(float(d @ d)) < STEP_TOL:
                stop = True
                break
            trial = P.apply(st, d)
            c, _ = truncated(P.residuals(trial, w), thr)
            evals += 1
            if c < cur:
                st, lam, taken = trial, max(lam / 10.0, LAMBDA_MIN), True
                break
            lam = lam * 10.0
        if stop or not taken:
            break
        steps += 1
        e, J = P.jacobian(st, w)
        cur, a = truncated(e, thr)
    return st, steps, evals, a, cost0, cur
