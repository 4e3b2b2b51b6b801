// Nonlinear refinement of a relative pose on the device: a Levenberg-Marquardt fit of (R, t) to the Sampson error of E = [t]x R
// under a hard-truncated loss - what the final refinement of PoseLib's estimate_relative_pose is, which the reference's second
// pose benchmark calls (romatch/benchmarks/megadepth_pose_estimation_benchmark_poselib.py).  It follows roma_op_essential +
// roma_op_recover_pose, whose pose is the winning five-point sample's.  tools/pose_refine_ref.py restates this file in numpy
// float64 expression by expression and is the oracle of the GPU tests.
//
//   residual    p = R (x, y, 1), l = t x p (= E x0h), q = (u, v, 1) x t, k = R^T q (= E^T x1h),
//               r = ((u l0 + v l1) + l2) / sqrt((l0^2 + l1^2) + (k0^2 + k1^2))
//   cost        sum of r^2 over the active rows (r^2 < thr^2) + thr^2 (n - active); a non-finite r is never active
//   parameters  R <- exp([w]x) R (Rodrigues), t <- normalise(t + d0 b0 + d1 b1), b0 = normalise(t x e_a) with a the axis of the
//               smallest |t_a| (first minimum), b1 = t x b0
//   Jacobian    dr = dc (1 / s) - r ((l0 dl0 + l1 dl1) + (k0 dk0 + k1 dk1)) (1 / den), s = sqrt(den), for the derivatives dl, dk, dc
//               of l, k and the numerator by each parameter
//   iteration   H = J^T J, g = J^T r over the active rows; (H + lambda diag H) delta = -g by Cholesky (not positive
//               definite: a pivot not above LM_PIVOT_REL times the largest diagonal entry); |delta| < LM_STEP_TOL stops; the
//               trial pose is accepted if its cost is lower (lambda <- max(lambda / 10, LM_LAMBDA_MIN)), else lambda <- 10 lambda
//               and the solve is repeated, at most LM_RETRIES times
//   stop        max_steps accepted steps, a short step, LM_RETRIES failed retries, fewer than LM_MIN_ROWS active rows (fewer rows
//               than parameters: H is singular; a start outside the threshold band usually has none), not positive definite.
//               The pose so far is returned: the cost never rises and a pose never turns into "not found".
//
// pose_refine_kernel: one workgroup of LM_THREADS per pair runs the whole loop in one launch.  Rows are strided over the threads;
// every thread sums its rows in ascending order, a wave adds its lanes by an xor butterfly (every lane ends with the same bits),
// the waves' sums go through LDS and are added in wave order by every thread.  So each thread holds the same H, g, cost and
// count, solves the same 5 x 5 system and takes the same branch: the pose lives in registers, nothing is handed off, and the
// only barriers are the two around the LDS exchange.  The order of every sum depends on LM_THREADS alone: results are
// bit-identical from run to run and independent of B.  The loop is bounded by max_steps x (1 + LM_RETRIES) cost evaluations.
// pose_refine_mask_kernel: grid (point blocks, pair): mask = active under the final pose and in front of both cameras (the
// linear triangulation of recoverPose, cheirality.h).
#include "pose_refine.h"

#include "cheirality.h"

namespace roma {
namespace {

constexpr int LM_THREADS = 512, LM_WAVES = LM_THREADS / 64;
constexpr int LM_SUMS = 21;               // H (upper triangle, row-major: 15), g (5), sum of r^2 over the active rows
constexpr double LM_LAMBDA0 = 1e-3, LM_LAMBDA_MIN = 1e-10;
constexpr int LM_RETRIES = 10;            // retries of one step with a ten times larger lambda
constexpr double LM_STEP_TOL = 1e-10;     // |delta| below which the fit has converged
constexpr double LM_PIVOT_REL = 1e-14;    // Cholesky pivot / largest diagonal entry of H + lambda diag H
constexpr int LM_MIN_ROWS = 5;            // rows of a pair, and active rows of an iteration, below which nothing is fitted
constexpr double LM_DIST = 1e9;           // distance_thresh of the cheirality test: what estimate_pose passes to recover_pose

struct LmState {                          // what the fit leaves for the mask kernel
  double c[12];                           // final R (row-major) and unit t, the layout cheiral() reads
  int n, valid;
};

struct LmRow {
  double p[3], l[3], q[3], k[2], den, s, r, inv_s, inv_den;
};

__device__ __forceinline__ void lm_row(const double* R, const double* t, float2 a, float2 b, LmRow& w) {
  const double x = a.x, y = a.y, u = b.x, v = b.y;
#pragma unroll
  for (int i = 0; i < 3; ++i) w.p[i] = (R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2];
  w.l[0] = t[1] * w.p[2] - t[2] * w.p[1];
  w.l[1] = t[2] * w.p[0] - t[0] * w.p[2];
  w.l[2] = t[0] * w.p[1] - t[1] * w.p[0];
  w.q[0] = v * t[2] - t[1];
  w.q[1] = t[0] - u * t[2];
  w.q[2] = u * t[1] - v * t[0];
#pragma unroll
  for (int j = 0; j < 2; ++j) w.k[j] = (R[j] * w.q[0] + R[3 + j] * w.q[1]) + R[6 + j] * w.q[2];
  const double c = (u * w.l[0] + v * w.l[1]) + w.l[2];
  w.den = (w.l[0] * w.l[0] + w.l[1] * w.l[1]) + (w.k[0] * w.k[0] + w.k[1] * w.k[1]);
  w.s = sqrt(w.den);
  w.r = c / w.s;
}

// dr of a parameter whose derivative of l is A x Bv and of q is dq
__device__ __forceinline__ double lm_col(const double* R, const LmRow& w, double u, double v, const double* A, const double* Bv,
                                         const double* dq) {
  const double dl0 = A[1] * Bv[2] - A[2] * Bv[1], dl1 = A[2] * Bv[0] - A[0] * Bv[2], dl2 = A[0] * Bv[1] - A[1] * Bv[0];
  const double dk0 = (R[0] * dq[0] + R[3] * dq[1]) + R[6] * dq[2];
  const double dk1 = (R[1] * dq[0] + R[4] * dq[1]) + R[7] * dq[2];
  const double dc = (u * dl0 + v * dl1) + dl2;
  return dc * w.inv_s - w.r * (((w.l[0] * dl0 + w.l[1] * dl1) + (w.k[0] * dk0 + w.k[1] * dk1)) * w.inv_den);
}

__device__ __forceinline__ void lm_basis(const double* t, double* b0, double* b1) {
  int a = 0;
  double m = fabs(t[0]);
  if (fabs(t[1]) < m) { a = 1; m = fabs(t[1]); }
  if (fabs(t[2]) < m) a = 2;
  // t x e_a
  double c0 = a == 0 ? 0.0 : a == 1 ? -t[2] : t[1];
  double c1 = a == 0 ? t[2] : a == 1 ? 0.0 : -t[0];
  double c2 = a == 0 ? -t[1] : a == 1 ? t[0] : 0.0;
  const double nrm = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  b0[0] = c0 / nrm; b0[1] = c1 / nrm; b0[2] = c2 / nrm;
  b1[0] = t[1] * b0[2] - t[2] * b0[1];
  b1[1] = t[2] * b0[0] - t[0] * b0[2];
  b1[2] = t[0] * b0[1] - t[1] * b0[0];
}

// the workgroup's totals of v[0 .. NV) and cnt in every thread: lanes by an xor butterfly, waves in order through LDS
template <int NV>
__device__ __forceinline__ void lm_reduce(double (&v)[NV], int& cnt, double* sh, int* shc) {
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
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = sh[k];
#pragma unroll
    for (int w = 1; w < LM_WAVES; ++w) s = s + sh[w * NV + k];
    v[k] = s;
  }
  int c = shc[0];
#pragma unroll
  for (int w = 1; w < LM_WAVES; ++w) c += shc[w];
  cnt = c;
}

// truncated cost of the pose (R, t) and its active rows
__device__ __forceinline__ double lm_cost(const double* R, const double* t, const float2* ka, const float2* kb, int n, double thr2,
                                          double* sh, int* shc, int& nact) {
  double s[1] = {0.0};
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    LmRow w;
    lm_row(R, t, ka[i], kb[i], w);
    const double r2 = w.r * w.r;
    const bool act = r2 < thr2;  // false for NaN
    s[0] = s[0] + (act ? r2 : 0.0);
    cnt += act ? 1 : 0;
  }
  lm_reduce(s, cnt, sh, shc);
  nact = cnt;
  return s[0] + thr2 * (double)(n - cnt);
}

// H (15), g (5) and the truncated cost at (R, t)
__device__ __forceinline__ double lm_normal(const double* R, const double* t, const float2* ka, const float2* kb, int n, double thr2,
                                            double* sh, int* shc, double (&acc)[LM_SUMS], int& nact) {
  double b0[3], b1[3];
  lm_basis(t, b0, b1);
#pragma unroll
  for (int k = 0; k < LM_SUMS; ++k) acc[k] = 0.0;
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    const float2 a = ka[i], b = kb[i];
    LmRow w;
    lm_row(R, t, a, b, w);
    const double r2 = w.r * w.r;
    if (r2 < thr2) {
      w.inv_s = 1.0 / w.s;  // two reciprocals instead of a division per column
      w.inv_den = 1.0 / w.den;
      const double u = b.x, v = b.y;
      const double* p = w.p;
      const double* q = w.q;
      double J[5];
      {  // rotation about e_i: dp = e_i x p, dq = q x e_i
        const double dp0[3] = {0.0, -p[2], p[1]}, dp1[3] = {p[2], 0.0, -p[0]}, dp2[3] = {-p[1], p[0], 0.0};
        const double dq0[3] = {0.0, q[2], -q[1]}, dq1[3] = {-q[2], 0.0, q[0]}, dq2[3] = {q[1], -q[0], 0.0};
        J[0] = lm_col(R, w, u, v, t, dp0, dq0);
        J[1] = lm_col(R, w, u, v, t, dp1, dq1);
        J[2] = lm_col(R, w, u, v, t, dp2, dq2);
      }
      {  // translation along b: dl = b x p, dq = x1h x b
        const double dq3[3] = {v * b0[2] - b0[1], b0[0] - u * b0[2], u * b0[1] - v * b0[0]};
        const double dq4[3] = {v * b1[2] - b1[1], b1[0] - u * b1[2], u * b1[1] - v * b1[0]};
        J[3] = lm_col(R, w, u, v, b0, p, dq3);
        J[4] = lm_col(R, w, u, v, b1, p, dq4);
      }
      int k = 0;
#pragma unroll
      for (int i2 = 0; i2 < 5; ++i2)
#pragma unroll
        for (int j2 = i2; j2 < 5; ++j2) {
          acc[k] = acc[k] + J[i2] * J[j2];
          ++k;
        }
#pragma unroll
      for (int i2 = 0; i2 < 5; ++i2) acc[15 + i2] = acc[15 + i2] + J[i2] * w.r;
      acc[20] = acc[20] + r2;
      ++cnt;
    }
  }
  lm_reduce(acc, cnt, sh, shc);
  nact = cnt;
  return acc[20] + thr2 * (double)(n - cnt);
}

// delta of (H + lam diag H) delta = -g by Cholesky; false when a pivot is not above LM_PIVOT_REL x the largest diagonal entry
__device__ __forceinline__ bool lm_solve(const double (&acc)[LM_SUMS], double lam, double (&d)[5]) {
  double A[5][5], L[5][5];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = i; j < 5; ++j) {
        A[i][j] = acc[k];
        A[j][i] = acc[k];
        ++k;
      }
  }
  double big = -INFINITY;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    A[i][i] = A[i][i] + lam * A[i][i];
    big = fmax(big, A[i][i]);
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj = dj - L[j][k] * L[j][k];
    ok = ok && dj > LM_PIVOT_REL * big;
    L[j][j] = sqrt(dj);
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  double y[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double s = -acc[15 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 4; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 5; ++k) s = s - L[k][i] * d[k];
    d[i] = s / L[i][i];
  }
  return ok;
}

// the pose after the step d = (w, d0, d1)
__device__ __forceinline__ void lm_apply(const double* R, const double* t, const double (&d)[5], double* Rn, double* tn) {
  double b0[3], b1[3];
  lm_basis(t, b0, b1);
  double t1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) t1[k] = (t[k] + d[3] * b0[k]) + d[4] * b1[k];
  const double nrm = sqrt((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) tn[k] = t1[k] / nrm;
  // exp([w]x) = I + a K + b K^2 with h = th / 2, s = sin(h) / h: a = sin(th) / th = s cos(h), b = (1 - cos(th)) / th^2 = s^2 / 2
  const double th2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  double a = 1.0, b = 0.5;
  if (!(th2 < 1e-30)) {
    const double h = 0.5 * sqrt(th2);
    double sn, cs;
    sincos(h, &sn, &cs);
    const double sh = sn / h;
    a = sh * cs;
    b = 0.5 * (sh * sh);
  }
  const double K[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
  double K2[9], M[9];
  mat3(K, K, K2);
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * K[k]) + b * K2[k];
  mat3(M, R, Rn);
}

__global__ __launch_bounds__(LM_THREADS) void pose_refine_kernel(const double* __restrict__ R_in, const double* __restrict__ t_in,
                                                                 const float2* __restrict__ kpts_a, const float2* __restrict__ kpts_b,
                                                                 const int* __restrict__ counts, const unsigned char* __restrict__ valid,
                                                                 int N, double thr, int max_steps, double* __restrict__ out_R,
                                                                 double* __restrict__ out_t, int* __restrict__ out_info,
                                                                 LmState* __restrict__ st) {
  __shared__ double sh[LM_WAVES * LM_SUMS];
  __shared__ int shc[LM_WAVES];
  const int b = blockIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  const float2* ka = kpts_a + (long)b * N;
  const float2* kb = kpts_b + (long)b * N;
  double R[9], t[3];
  bool ok = (!valid || valid[b]) && n >= LM_MIN_ROWS;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    R[k] = R_in[(long)b * 9 + k];
    ok = ok && isfinite(R[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t[k] = t_in[(long)b * 3 + k];
    ok = ok && isfinite(t[k]);
  }
  const double tnorm = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  ok = ok && tnorm > 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = t[k] / tnorm;
  if (threadIdx.x == 0) {  // stored here so that the flag is not carried through the loop
    out_info[b * 4 + 3] = ok ? 1 : 0;
    st[b].n = n;
    st[b].valid = ok ? 1 : 0;
  }
  int steps = 0, evals = 0, nact = 0;
  if (ok) {  // uniform over the workgroup, like every branch below: all threads hold the same values
    const double thr2 = thr * thr;
    double acc[LM_SUMS];
    double lam = LM_LAMBDA0;
    double cur = lm_normal(R, t, ka, kb, n, thr2, sh, shc, acc, nact);
    evals = 1;
    bool go = true;
    while (go && steps < max_steps && nact >= LM_MIN_ROWS) {
      bool taken = false;
      for (int tr = 0; tr <= LM_RETRIES && go && !taken; ++tr) {
        double d[5], Rn[9], tn[3];
        const bool pd = lm_solve(acc, lam, d);
        const double len = sqrt((((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]) + d[4] * d[4]);
        if (!pd || len < LM_STEP_TOL) {
          go = false;
        } else {
          lm_apply(R, t, d, Rn, tn);
          int na;
          const double c = lm_cost(Rn, tn, ka, kb, n, thr2, sh, shc, na);
          ++evals;
          if (c < cur) {
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = tn[k];
            lam = fmax(lam / 10.0, LM_LAMBDA_MIN);
            taken = true;
          } else {
            lam = lam * 10.0;
          }
        }
      }
      if (!taken) break;
      ++steps;
      cur = lm_normal(R, t, ka, kb, n, thr2, sh, shc, acc, nact);
    }
  }
  if (threadIdx.x == 0) {
    // without an accepted step the input comes back untouched, whatever the norm of its t (read again: not kept in registers)
    for (int k = 0; k < 9; ++k) out_R[(long)b * 9 + k] = steps ? R[k] : R_in[(long)b * 9 + k];
    for (int k = 0; k < 3; ++k) out_t[(long)b * 3 + k] = steps ? t[k] : t_in[(long)b * 3 + k];
    out_info[b * 4] = steps;
    out_info[b * 4 + 1] = evals;
    out_info[b * 4 + 2] = nact;
    LmState& S = st[b];
    for (int k = 0; k < 9; ++k) S.c[k] = R[k];
    for (int k = 0; k < 3; ++k) S.c[9 + k] = t[k];
  }
}

// grid (ceil(N / 256), B): mask[b, i] = active under the final pose and in front of both cameras
__global__ __launch_bounds__(256) void pose_refine_mask_kernel(const float2* __restrict__ kpts_a, const float2* __restrict__ kpts_b, int N,
                                                               double thr, const LmState* __restrict__ st,
                                                               unsigned char* __restrict__ mask) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const LmState& S = st[b];
  bool in = false;
  if (S.valid && i < S.n) {
    const float2 a = kpts_a[(long)b * N + i], q = kpts_b[(long)b * N + i];
    LmRow w;
    lm_row(S.c, S.c + 9, a, q, w);
    in = w.r * w.r < thr * thr && cheiral(S.c, a.x, a.y, q.x, q.y, LM_DIST);
  }
  mask[(long)b * N + i] = in ? 1 : 0;
}

}  // namespace

size_t refine_pose_workspace_bytes(int B, int N) { return B > 0 && N > 0 ? align256(sizeof(LmState) * (size_t)B) + 256 : 0; }

int refine_pose_launch(const double* R, const double* t, const float* kpts_a, const float* kpts_b, const int* counts,
                       const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_r, double* out_t,
                       unsigned char* out_mask, int* out_info, void* ws, size_t ws_bytes, hipStream_t s) {
  ROMA_REQUIRE(R && t && kpts_a && kpts_b && out_r && out_t && out_mask && out_info && ws, "refine_pose: null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16), "refine_pose: need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(thr > 0 && isfinite(thr), "refine_pose: threshold must be positive and finite");
  ROMA_REQUIRE(max_steps >= 0 && max_steps <= (1 << 16), "refine_pose: need 0 <= max_steps <= 65536");
  ROMA_REQUIRE(ws_bytes >= refine_pose_workspace_bytes(B, N), "refine_pose: workspace too small (roma_op_refine_pose_workspace)");
  LmState* st = align_base<LmState*>(ws);
  const float2* ka = reinterpret_cast<const float2*>(kpts_a);
  const float2* kb = reinterpret_cast<const float2*>(kpts_b);
  hipLaunchKernelGGL(pose_refine_kernel, dim3(B), dim3(LM_THREADS), 0, s, R, t, ka, kb, counts, valid, N, thr, max_steps, out_r, out_t,
                     out_info, st);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(pose_refine_mask_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, ka, kb, N, thr, st, out_mask);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
