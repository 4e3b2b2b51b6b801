// Nonlinear refinement of a relative pose on the device: a Levenberg-Marquardt fit of (R, t) to the Sampson error of E = [t]x R
// under a hard-truncated loss - what the final refinement of PoseLib's estimate_relative_pose is, which the reference's second
// pose benchmark calls (romatch/benchmarks/megadepth_pose_estimation_benchmark_poselib.py).  It follows roma_op_essential +
// roma_op_recover_pose, whose pose is the winning five-point sample's.  tools/pose_refine_ref.py restates this file in numpy
// float64 expression by expression and is the oracle of the GPU tests.
//
// The loop - cost, iteration, stopping rules, the reduction and its fixed order - is lm_fit<P> of lm_fit.h, which this file
// shares with model_refine.hip.  PoseFit is its policy (5 parameters, one residual, the points as they are):
//
//   residual    p = R (x, y, 1), l = t x p (= E x0h), q = (u, v, 1) x t, k = R^T q (= E^T x1h),
//               r = ((u l0 + v l1) + l2) / sqrt((l0^2 + l1^2) + (k0^2 + k1^2))
//   parameters  R <- exp([w]x) R (Rodrigues), t <- normalise(t + d0 b0 + d1 b1), b0 = normalise(t x e_a) with a the axis of the
//               smallest |t_a| (first minimum), b1 = t x b0
//   Jacobian    dr = dc (1 / s) - r ((l0 dl0 + l1 dl1) + (k0 dk0 + k1 dk1)) (1 / den), s = sqrt(den), for the derivatives dl, dk, dc
//               of l, k and the numerator by each parameter
//
// pose_refine_kernel: one workgroup of LM_THREADS per pair checks the start, runs lm_fit<PoseFit> and stores the pose.
// pose_refine_mask_kernel: grid (point blocks, pair): mask = active under the final pose and in front of both cameras (the
// linear triangulation of recoverPose, cheirality.h).
#include "../../include/roma_hip.h"
#include "cheirality.h"
#include "lm_fit.h"

namespace roma {
namespace {

constexpr double LM_DIST = 1e9;           // distance_thresh of the cheirality test: what estimate_pose passes to recover_pose

struct LmState {                          // what the fit leaves for the mask kernel
  double c[12];                           // final R (row-major) and unit t, the layout cheiral() reads
  int n, valid;
};

struct PoseFit {
  static constexpr int NP = 5, NR = 1, MIN_ROWS = 5;
  struct State { double R[9], t[3]; };
  struct Prep {};
  struct Aux { double R[9], t[3], b0[3], b1[3]; };  // b0, b1: the tangent basis of t, the directions of d0 and d1
  struct Row { double p[3], l[3], q[3], k[2], den, s, r; };

  __device__ static LmPoint point(const Prep&, float2 a, float2 b) { return {a.x, a.y, b.x, b.y}; }

  __device__ static void basis(const double* t, double* b0, double* b1) {
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

  __device__ static void aux(const State& s, const Prep&, Aux& ax) {
#pragma unroll
    for (int k = 0; k < 9; ++k) ax.R[k] = s.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ax.t[k] = s.t[k];
    basis(s.t, ax.b0, ax.b1);
  }

  // the Sampson distance of a row under (R, t), squared; its parts in w
  __device__ static double sampson(const double* R, const double* t, const LmPoint& z, Row& w) {
    const double x = z.x, y = z.y, u = z.u, v = z.v;
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
    return w.r * w.r;
  }
  __device__ static double residual(const Aux& ax, const LmPoint& z, Row& w, double (&e)[NR]) {
    const double r2 = sampson(ax.R, ax.t, z, w);
    e[0] = w.r;
    return r2;
  }

  // dr of a parameter whose derivative of l is A x Bv and of q is dq
  __device__ static double col(const double* R, const Row& w, double inv_s, double inv_den, double u, double v, const double* A,
                               const double* Bv, const double* dq) {
    const double dl0 = A[1] * Bv[2] - A[2] * Bv[1], dl1 = A[2] * Bv[0] - A[0] * Bv[2], dl2 = A[0] * Bv[1] - A[1] * Bv[0];
    const double dk0 = (R[0] * dq[0] + R[3] * dq[1]) + R[6] * dq[2];
    const double dk1 = (R[1] * dq[0] + R[4] * dq[1]) + R[7] * dq[2];
    const double dc = (u * dl0 + v * dl1) + dl2;
    return dc * inv_s - w.r * (((w.l[0] * dl0 + w.l[1] * dl1) + (w.k[0] * dk0 + w.k[1] * dk1)) * inv_den);
  }

  __device__ static void jacobian(const State&, const Aux& ax, const LmPoint& z, const Row& w, const double (&e)[NR],
                                  double (&J)[NR][NP]) {
    const double inv_s = 1.0 / w.s, inv_den = 1.0 / w.den;  // two reciprocals instead of a division per column
    const double u = z.u, v = z.v;
    const double* R = ax.R;
    const double* t = ax.t;
    const double* b0 = ax.b0;
    const double* b1 = ax.b1;
    const double* p = w.p;
    const double* q = w.q;
    {  // rotation about e_i: dp = e_i x p, dq = q x e_i
      const double dp0[3] = {0.0, -p[2], p[1]}, dp1[3] = {p[2], 0.0, -p[0]}, dp2[3] = {-p[1], p[0], 0.0};
      const double dq0[3] = {0.0, q[2], -q[1]}, dq1[3] = {-q[2], 0.0, q[0]}, dq2[3] = {q[1], -q[0], 0.0};
      J[0][0] = col(R, w, inv_s, inv_den, u, v, t, dp0, dq0);
      J[0][1] = col(R, w, inv_s, inv_den, u, v, t, dp1, dq1);
      J[0][2] = col(R, w, inv_s, inv_den, u, v, t, dp2, dq2);
    }
    {  // translation along b: dl = b x p, dq = x1h x b
      const double dq3[3] = {v * b0[2] - b0[1], b0[0] - u * b0[2], u * b0[1] - v * b0[0]};
      const double dq4[3] = {v * b1[2] - b1[1], b1[0] - u * b1[2], u * b1[1] - v * b1[0]};
      J[0][3] = col(R, w, inv_s, inv_den, u, v, b0, p, dq3);
      J[0][4] = col(R, w, inv_s, inv_den, u, v, b1, p, dq4);
    }
  }

  // the pose after the step d = (w, d0, d1)
  __device__ static void apply(const State& s, const double (&d)[NP], State& o) {
    double b0[3], b1[3];
    basis(s.t, b0, b1);
    double t1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) t1[k] = (s.t[k] + d[3] * b0[k]) + d[4] * b1[k];
    const double nrm = sqrt((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.t[k] = t1[k] / nrm;
    double E[9];
    lm_rodrigues(d[0], d[1], d[2], E);
    mat3(E, s.R, o.R);
  }
};

__global__ __launch_bounds__(LM_THREADS) void pose_refine_kernel(const double* __restrict__ R_in, const double* __restrict__ t_in,
                                                                 const float2* __restrict__ kpts_a, const float2* __restrict__ kpts_b,
                                                                 const int* __restrict__ counts, const unsigned char* __restrict__ valid,
                                                                 int N, double thr, int max_steps, double* __restrict__ out_R,
                                                                 double* __restrict__ out_t, int* __restrict__ out_info,
                                                                 LmState* __restrict__ st) {
  __shared__ double shn[LM_WAVES * lm_sums(PoseFit::NP)];  // the waves' sums of the normal equations
  __shared__ double sh[LM_WAVES];                          // every other exchange
  __shared__ int shc[LM_WAVES];
  const int b = blockIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  const float2* ka = kpts_a + (long)b * N;
  const float2* kb = kpts_b + (long)b * N;
  PoseFit::State S;
  bool ok = (!valid || valid[b]) && n >= PoseFit::MIN_ROWS;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    S.R[k] = R_in[(long)b * 9 + k];
    ok = ok && isfinite(S.R[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    S.t[k] = t_in[(long)b * 3 + k];
    ok = ok && isfinite(S.t[k]);
  }
  const double tnorm = sqrt((S.t[0] * S.t[0] + S.t[1] * S.t[1]) + S.t[2] * S.t[2]);
  ok = ok && tnorm > 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) S.t[k] = S.t[k] / tnorm;
  if (threadIdx.x == 0) {  // stored here so that the flag is not carried through the loop
    out_info[b * 4 + 3] = ok ? 1 : 0;
    st[b].n = n;
    st[b].valid = ok ? 1 : 0;
  }
  LmResult fit = {0, 0, 0, NAN, NAN};
  // uniform over the workgroup, like every branch of the loop: all threads hold the same values
  if (ok) fit = lm_fit<PoseFit>(S, PoseFit::Prep(), ka, kb, n, thr * thr, max_steps, shn, sh, shc);
  if (threadIdx.x == 0) {
    // without an accepted step the input comes back untouched, whatever the norm of its t (read again: not kept in registers)
    for (int k = 0; k < 9; ++k) out_R[(long)b * 9 + k] = fit.steps ? S.R[k] : R_in[(long)b * 9 + k];
    for (int k = 0; k < 3; ++k) out_t[(long)b * 3 + k] = fit.steps ? S.t[k] : t_in[(long)b * 3 + k];
    out_info[b * 4] = fit.steps;
    out_info[b * 4 + 1] = fit.evals;
    out_info[b * 4 + 2] = fit.nact;
    LmState& T = st[b];
    for (int k = 0; k < 9; ++k) T.c[k] = S.R[k];
    for (int k = 0; k < 3; ++k) T.c[9 + k] = S.t[k];
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
    PoseFit::Row w;
    const double r2 = PoseFit::sampson(S.c, S.c + 9, PoseFit::point(PoseFit::Prep(), a, q), w);
    in = r2 < thr * thr && cheiral(S.c, a.x, a.y, q.x, q.y, LM_DIST);
  }
  mask[(long)b * N + i] = in ? 1 : 0;
}

// the workspace is the pairs' states; returns its bytes
size_t pose_refine_carve(Workspace256 ws, int B, LmState*& st) {
  st = ws.take<LmState>(B);
  return ws.bytes();
}

}  // namespace

extern "C" long roma_op_refine_pose_workspace(int B, int N) {
  LmState* st;
  return B > 0 && N > 0 ? pose_refine_carve(Workspace256(), B, st) : 0;
}

extern "C" int roma_op_refine_pose(const double* R, const double* t, const float* kpts_a, const float* kpts_b, const int* counts,
                                   const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_r, double* out_t,
                                   unsigned char* out_mask, int* out_info, void* ws, long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(R && t && kpts_a && kpts_b && out_r && out_t && out_mask && out_info && ws, "refine_pose: null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16), "refine_pose: need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(thr > 0 && isfinite(thr), "refine_pose: threshold must be positive and finite");
  ROMA_REQUIRE(max_steps >= 0 && max_steps <= (1 << 16), "refine_pose: need 0 <= max_steps <= 65536");
  ROMA_REQUIRE(ws_bytes >= (size_t)roma_op_refine_pose_workspace(B, N), "refine_pose: workspace too small (roma_op_refine_pose_workspace)");
  LmState* st;
  pose_refine_carve(Workspace256(ws), B, st);
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
