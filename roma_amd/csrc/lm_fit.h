// The Levenberg-Marquardt loop of the refinement kernels: pose_refine.hip (PoseFit) and model_refine.hip (HomographyFit,
// FundamentalFit) run it through lm_fit<P>.  ransac.h first: its fp-contract setting holds here as well.
//
//   cost        sum of |r|^2 over the active rows (|r|^2 < thr^2) + thr^2 (n - active); a non-finite residual is never active;
//               thr^2 = inf: plain least squares over the finite rows, the second term is dropped
//   iteration   H = J^T J, g = J^T r over the active rows; (H + lambda diag H) delta = -g by Cholesky (not positive definite: a
//               pivot not above LM_PIVOT_REL times the largest diagonal entry); |delta| < LM_STEP_TOL stops; the trial state is
//               accepted if its cost is lower (lambda <- max(lambda / 10, LM_LAMBDA_MIN)), else lambda <- 10 lambda and the
//               solve is repeated, at most LM_RETRIES times
//   stop        max_steps accepted steps, a short step, LM_RETRIES failed retries, fewer than P::MIN_ROWS active rows (fewer
//               rows than parameters: H is singular; a start outside the threshold band usually has none), not positive
//               definite.  The state so far is returned: the cost never rises and a model never turns into "not found".
//
// One workgroup of LM_THREADS per pair runs the whole loop.  Rows are strided over the threads; every thread sums its rows in
// ascending order, a wave adds its lanes by an xor butterfly (every lane ends with the same bits), the waves' sums go through
// LDS and are added in wave order by every thread.  So each thread holds the same normal equations, solves the same system in
// registers and takes the same branch: the state lives in registers, nothing is handed off, no atomics, and the only barriers
// are the two around each LDS exchange.  The order of every sum depends on LM_THREADS alone: results are bit-identical from
// run to run, independent of B and of the pair's place in the batch.  The loop is bounded by max_steps x (1 + LM_RETRIES) cost
// evaluations.
// LM_THREADS = 512 is two waves per SIMD and 256 VGPRs per thread.  The homography's 45 f64 accumulators take 90 of them in the
// row loop and the 8 x 8 Cholesky factor 72 in the solve, so the waves' sums of H and g stay in LDS, where the exchange puts
// them anyway, and the solve and its retries add them up from there: with the totals held in registers across the solve the
// kernel spilled at 512 threads (27 VGPRs) and fitted only at 256, where a pass over the rows takes twice as long.
//
// A policy P supplies
//   NP, NR, MIN_ROWS   parameters, residuals per row, rows of a pair and active rows of an iteration below which nothing is fitted
//   State              the parametrised model
//   Prep               what is fixed for the pair and a row evaluation reads (the Hartley normalisation; empty for the pose)
//   Aux                what a row evaluation reads of a state, computed once per state by aux(state, prep, Aux&), never per row
//   Row                what the Jacobian reuses of the residual
//   point(prep, a, b)                   the row as the fit sees it (LmPoint), from one float2 of each row array
//   row(prep, ka, kb, i)                optional, instead of point: row i read by the policy itself from the two arrays, in
//                                       a layout and a point type of its own (absolute_pose.hip: 3-D points of three floats)
//   residual(aux, point, Row&, e[NR])   the residuals of a row; returns |e|^2
//   jacobian(state, aux, point, row, e, J[NR][NP])
//   apply(state, delta[NP], State&)     the state after a step
#pragma once
#include <type_traits>

#include "ransac.h"

namespace roma {
namespace {

constexpr int LM_THREADS = 512, LM_WAVES = LM_THREADS / 64;
constexpr double LM_LAMBDA0 = 1e-3, LM_LAMBDA_MIN = 1e-10;
constexpr int LM_RETRIES = 10;            // retries of one step with a ten times larger lambda
constexpr double LM_STEP_TOL = 1e-10;     // |delta| below which the fit has converged
constexpr double LM_PIVOT_REL = 1e-14;    // Cholesky pivot / largest diagonal entry of H + lambda diag H

// sums of the normal equations of NP parameters: H (upper triangle, row-major), g, sum of |r|^2 over the active rows
constexpr int lm_sums(int NP) { return NP * (NP + 1) / 2 + NP + 1; }

struct LmPoint {
  double x, y, u, v;
};

// where lm_fit gets row i from: P::row if the policy has one, else P::point on ka[i], kb[i]
template <class P, class = void>
struct LmRows {
  __device__ static __forceinline__ LmPoint get(const typename P::Prep& q, const float2* ka, const float2* kb, int i) {
    return P::point(q, ka[i], kb[i]);
  }
};
template <class P>
struct LmRows<P, std::void_t<decltype(&P::row)>> {
  __device__ static __forceinline__ auto get(const typename P::Prep& q, const float2* ka, const float2* kb, int i) {
    return P::row(q, ka, kb, i);
  }
};

struct LmResult {
  int steps, evals, nact;  // accepted steps, cost evaluations, active rows at the end
  double cost0, cost;      // truncated cost at the start and at the end
};

// exp([w]x) = I + a K + b K^2 with h = th / 2, s = sin(h) / h: a = sin(th) / th = s cos(h), b = (1 - cos(th)) / th^2 = s^2 / 2
__device__ __forceinline__ void lm_rodrigues(double w0, double w1, double w2, double* M) {
  const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
  double a = 1.0, b = 0.5;
  if (!(th2 < 1e-30)) {
    const double h = 0.5 * sqrt(th2);
    double sn, cs;
    sincos(h, &sn, &cs);
    const double sh = sn / h;
    a = sh * cs;
    b = 0.5 * (sh * sh);
  }
  const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  double K2[9];
  mat3(K, K, K2);
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * K[k]) + b * K2[k];
}

// the per-wave sums of v[0 .. NV) and cnt into LDS: lanes by an xor butterfly, one row of sh per wave.  The totals are read
// back by lm_total_of / lm_count, which add the waves in order - in every thread, so all threads hold the same bits.
template <int NV>
__device__ __forceinline__ void lm_exchange(double (&v)[NV], int cnt, double* sh, int* shc) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] = v[k] + __shfl_xor(v[k], off, 64);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // the previous exchange has been read
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) sh[wave * NV + k] = v[k];
    shc[wave] = cnt;
  }
  __syncthreads();
}

template <int NV>
__device__ __forceinline__ double lm_total_of(const double* sh, int k) {
  double s = sh[k];
#pragma unroll
  for (int w = 1; w < LM_WAVES; ++w) s = s + sh[w * NV + k];
  return s;
}

__device__ __forceinline__ int lm_count(const int* shc) {
  int c = shc[0];
#pragma unroll
  for (int w = 1; w < LM_WAVES; ++w) c += shc[w];
  return c;
}

// the workgroup's totals of v[0 .. NV) and cnt in every thread
template <int NV>
__device__ __forceinline__ void lm_reduce(double (&v)[NV], int& cnt, double* sh, int* shc) {
  lm_exchange(v, cnt, sh, shc);
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = lm_total_of<NV>(sh, k);
  cnt = lm_count(shc);
}

__device__ __forceinline__ double lm_total(double sum, double thr2, int n, int cnt) {
  return isfinite(thr2) ? sum + thr2 * (double)(n - cnt) : sum;
}

// truncated cost of the state behind ax and its active rows
template <class P>
__device__ __forceinline__ double lm_cost(const typename P::Aux& ax, const typename P::Prep& q, const float2* ka, const float2* kb,
                                          int n, double thr2, double* sh, int* shc, int& nact) {
  double s[1] = {0.0};
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    const auto w = LmRows<P>::get(q, ka, kb, i);
    typename P::Row r;
    double e[P::NR];
    const double r2 = P::residual(ax, w, r, e);
    const bool act = r2 < thr2;  // false for NaN
    s[0] = s[0] + (act ? r2 : 0.0);
    cnt += act ? 1 : 0;
  }
  lm_reduce(s, cnt, sh, shc);
  nact = cnt;
  return lm_total(s[0], thr2, n, cnt);
}

// H (upper triangle, row-major), g and the truncated cost at st.  The waves' sums of H and g stay in shn for lm_solve, which
// may run several times (retries) before the next call replaces them: the accumulators are live in the row loop only.
template <class P, int NS>
__device__ __forceinline__ double lm_normal(const typename P::State& st, const typename P::Aux& ax, const typename P::Prep& q,
                                            const float2* ka, const float2* kb, int n, double thr2, double* shn, int* shc,
                                            int& nact) {
  constexpr int NP = P::NP, NH = NP * (NP + 1) / 2;
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    const auto w = LmRows<P>::get(q, ka, kb, i);
    typename P::Row r;
    double e[P::NR];
    const double r2 = P::residual(ax, w, r, e);
    if (r2 < thr2) {
      double J[P::NR][NP];
      P::jacobian(st, ax, w, r, e, J);
#pragma unroll
      for (int c = 0; c < P::NR; ++c) {
        int k = 0;
#pragma unroll
        for (int i2 = 0; i2 < NP; ++i2)
#pragma unroll
          for (int j2 = i2; j2 < NP; ++j2) {
            acc[k] = acc[k] + J[c][i2] * J[c][j2];
            ++k;
          }
#pragma unroll
        for (int i2 = 0; i2 < NP; ++i2) acc[NH + i2] = acc[NH + i2] + J[c][i2] * e[c];
      }
      acc[NH + NP] = acc[NH + NP] + r2;
      ++cnt;
    }
  }
  lm_exchange(acc, cnt, shn, shc);
  nact = lm_count(shc);
  return lm_total(lm_total_of<NS>(shn, NH + NP), thr2, n, nact);
}

// delta of (H + lam diag H) delta = -g by Cholesky; false when a pivot is not above LM_PIVOT_REL x the largest diagonal entry
template <int NP, int NS>
__device__ __forceinline__ bool lm_solve(const double* shn, double lam, double (&d)[NP]) {
  constexpr int NH = NP * (NP + 1) / 2;
  double A[NP][NP], L[NP][NP];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
      for (int j = i; j < NP; ++j) {
        A[i][j] = lm_total_of<NS>(shn, k);
        A[j][i] = A[i][j];
        ++k;
      }
  }
  double big = -INFINITY;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    A[i][i] = A[i][i] + lam * A[i][i];
    big = fmax(big, A[i][i]);
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj = dj - L[j][k] * L[j][k];
    ok = ok && dj > LM_PIVOT_REL * big;
    L[j][j] = sqrt(dj);
#pragma unroll
    for (int i = j + 1; i < NP; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  double y[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double s = -lm_total_of<NS>(shn, NH + i);
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < NP; ++k) s = s - L[k][i] * d[k];
    d[i] = s / L[i][i];
  }
  return ok;
}

// The whole fit from the start S, which becomes the final state.  shn [LM_WAVES * lm_sums(P::NP)] holds the waves' sums of the
// normal equations across the retries of a step, sh [LM_WAVES] and shc [LM_WAVES] every other exchange.  Every branch is
// uniform over the workgroup: all threads hold the same values.
template <class P>
__device__ __forceinline__ LmResult lm_fit(typename P::State& S, const typename P::Prep& q, const float2* ka, const float2* kb, int n,
                                           double thr2, int max_steps, double* shn, double* sh, int* shc) {
  constexpr int NP = P::NP, NS = lm_sums(NP);
  typename P::Aux ax;
  int steps = 0, nact = 0;
  double lam = LM_LAMBDA0;
  P::aux(S, q, ax);
  double cur = lm_normal<P, NS>(S, ax, q, ka, kb, n, thr2, shn, shc, nact);
  const double cost0 = cur;
  int evals = 1;
  bool go = true;
  while (go && steps < max_steps && nact >= P::MIN_ROWS) {
    bool taken = false;
    for (int tr = 0; tr <= LM_RETRIES && go && !taken; ++tr) {
      double d[NP];
      const bool pd = lm_solve<NP, NS>(shn, lam, d);
      double len = 0.0;
#pragma unroll
      for (int k = 0; k < NP; ++k) len = len + d[k] * d[k];
      if (!pd || sqrt(len) < LM_STEP_TOL) {
        go = false;
      } else {
        typename P::State Sn;
        typename P::Aux axn;
        P::apply(S, d, Sn);
        P::aux(Sn, q, axn);
        int na;
        const double c = lm_cost<P>(axn, q, ka, kb, n, thr2, sh, shc, na);
        ++evals;
        if (c < cur) {
          S = Sn;
          lam = fmax(lam / 10.0, LM_LAMBDA_MIN);
          taken = true;
        } else {
          lam = lam * 10.0;
        }
      }
    }
    if (!taken) break;
    ++steps;
    P::aux(S, q, ax);
    cur = lm_normal<P, NS>(S, ax, q, ka, kb, n, thr2, shn, shc, nact);
  }
  return {steps, evals, nact, cost0, cur};
}

}  // namespace
}  // namespace roma
