// The 3-D point of every track from all the views that observe it, the poses given (roma_op_triangulate_views): the point half
// of bundle_adjust, and what gives it a start for more than two views.  x_cam = R X + t.  tools/triangulate_views_ref.py restates
// this file operation by operation in numpy float64 and is the oracle of tests/test_gpu_views.py.
//
// Per point, with the observations in use U (finite, of a valid view, not trimmed), x_n = ((u - cx) / fx, (v - cy) / fy):
//   start     fewer than min_views in U: DEGENERATE.  Ray d_v = R_v^T (x_n, 1) / |.| from the centre c_v = -R_v^T t_v; the midpoint
//             (sum (I - d d^T)) X = sum (I - d d^T) c by a 3 x 3 Cholesky factor; a pivot that is not finite or not above
//             LM_PIVOT_REL x the largest diagonal entry (parallel rays): DEGENERATE
//   refine    up to gn_steps Gauss-Newton steps on sum |p_xy / z - x_n|^2, p = R_v X + t_v, over U: analytic Jacobian, normal
//             equations by the same factor; a step is kept only when its cost is finite and strictly lower, the first one
//             that is not (or whose factor fails) ends the loop - the cost never rises above the midpoint's
//   trim      e_v = |error| / thr_v, thr_v = max_reproj / ((fx_v + fy_v) / 2); when trim is on, the largest e_v is above 1 and U
//             holds at least three, the worst observation (the lowest view of a tie) leaves U and the point starts again
// One thread per point; the views of the problem (pose, centre, camera, threshold) are staged once per workgroup in LDS and the
// observations are re-read from memory where they are used, so no per-thread array is indexed by a view.  `stats` is added over
// the workgroup in lane and wave order, then by one integer atomic per counter: bit-identical from run to run.
#include <math.h>
#include <stdint.h>

#include "../../include/roma_hip.h"
#include "common.h"
#include "tracks.h"
#include "triangulate.h"

// nothing here is fused: tools/triangulate_views_ref.py evaluates the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int TRIANGULATE_VIEWS_STATS = 8;    // ints per problem in roma_op_triangulate_views' out_stats
constexpr int TRIANGULATE_VIEWS_MAX_GN = 10;  // Gauss-Newton steps per fit
constexpr int TV_THREADS = 256, TV_WAVES = TV_THREADS / 64;
constexpr int TV_VIEW = 20;  // doubles of a view in LDS: R (9, row-major), t (3), centre (3), fx, fy, cx, cy, thr
constexpr int TV_T = 9, TV_C = 12, TV_FX = 15, TV_FY = 16, TV_CX = 17, TV_CY = 18, TV_THR = 19;
constexpr double TV_PIVOT_REL = 1e-14;            // lm_fit.h: LM_PIVOT_REL
constexpr double TV_RAD_TO_DEG = 57.29577951308232;  // 180 / pi

struct TvParams {
  const float2* kpts;
  const double* K;
  const double* R;
  const double* t;
  const unsigned char* view_valid;
  const int* counts;
  const unsigned char* valid;
  int V, N, min_views, gn_steps, trim;
  double max_reproj, min_parallax, max_depth;
  double* points;
  float* reproj;
  unsigned char* used;
  float* parallax;
  unsigned char* flags;
  int* stats;
};

__device__ __forceinline__ bool tv_seen(float2 k) { return isfinite(k.x) && isfinite(k.y); }

__device__ __forceinline__ void tv_normalise(const double* w, float2 k, double& x0, double& x1) {
  x0 = ((double)k.x - w[TV_CX]) / w[TV_FX];
  x1 = ((double)k.y - w[TV_CY]) / w[TV_FY];
}

// unit ray of the observation in the world frame
__device__ __forceinline__ void tv_ray(const double* w, float2 k, double (&d)[3]) {
  double x0, x1;
  tv_normalise(w, k, x0, x1);
  const double r0 = (w[0] * x0 + w[3] * x1) + w[6];
  const double r1 = (w[1] * x0 + w[4] * x1) + w[7];
  const double r2 = (w[2] * x0 + w[5] * x1) + w[8];
  const double nrm = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
  d[0] = r0 / nrm;
  d[1] = r1 / nrm;
  d[2] = r2 / nrm;
}

struct TvRes {
  double e0, e1, z, iz, ax, ay;
};

__device__ __forceinline__ TvRes tv_residual(const double* w, float2 k, const double (&X)[3]) {
  double x0, x1, p[3];
  tv_normalise(w, k, x0, x1);
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = ((w[3 * i] * X[0] + w[3 * i + 1] * X[1]) + w[3 * i + 2] * X[2]) + w[TV_T + i];
  TvRes r;
  r.z = p[2];
  r.iz = 1.0 / p[2];
  r.ax = p[0] * r.iz;
  r.ay = p[1] * r.iz;
  r.e0 = r.ax - x0;
  r.e1 = r.ay - x1;
  return r;
}

// x of A x = b, A the upper triangle (00, 01, 02, 11, 12, 22); false when a pivot is not finite or not above TV_PIVOT_REL x
// the largest diagonal entry
__device__ __forceinline__ bool tv_solve(const double (&A)[6], const double (&b)[3], double (&x)[3]) {
  const double piv = TV_PIVOT_REL * fmax(fmax(A[0], A[3]), A[5]);
  bool ok = A[0] > piv && isfinite(A[0]);
  const double l00 = sqrt(A[0]), l10 = A[1] / l00, l20 = A[2] / l00;
  const double p1 = A[3] - l10 * l10;
  ok = ok && p1 > piv && isfinite(p1);
  const double l11 = sqrt(p1), l21 = (A[4] - l20 * l10) / l11;
  const double p2 = (A[5] - l20 * l20) - l21 * l21;
  ok = ok && p2 > piv && isfinite(p2);
  const double l22 = sqrt(p2);
  const double y0 = b[0] / l00, y1 = (b[1] - l10 * y0) / l11, y2 = ((b[2] - l20 * y0) - l21 * y1) / l22;
  x[2] = y2 / l22;
  x[1] = (y1 - l21 * x[2]) / l11;
  x[0] = ((y0 - l10 * x[1]) - l20 * x[2]) / l00;
  return ok;
}

struct TvCtx {
  const double* vw;   // LDS [V][TV_VIEW]
  const float2* kp;   // the point's observation in view 0; view v is kp[v * N]
  int V, N;
  double max_depth;
};

// cost of X over the views of m; worst: the largest error in units of its view's threshold, wi its view (-1: none above 0);
// cheir: a view of m where not 0 < z < max_depth
__device__ __forceinline__ double tv_cost(const TvCtx& c, unsigned m, const double (&X)[3], double& worst, int& wi, bool& cheir) {
  double cost = 0.0;
  worst = 0.0;
  wi = -1;
  cheir = false;
#pragma unroll 1
  for (int v = 0; v < c.V; ++v) {
    if (!((m >> v) & 1u)) continue;
    const double* w = c.vw + v * TV_VIEW;
    const TvRes r = tv_residual(w, c.kp[(long)v * c.N], X);
    const double e2 = r.e0 * r.e0 + r.e1 * r.e1;
    cost = cost + e2;
    const double rel = sqrt(e2) / w[TV_THR];
    if (rel > worst) {
      worst = rel;
      wi = v;
    }
    if (!(r.z > 0.0 && r.z < c.max_depth)) cheir = true;
  }
  return cost;
}

// the midpoint of the rays of m; false: degenerate
__device__ __forceinline__ bool tv_midpoint(const TvCtx& c, unsigned m, double (&X)[3]) {
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int v = 0; v < c.V; ++v) {
    if (!((m >> v) & 1u)) continue;
    const double* w = c.vw + v * TV_VIEW;
    double d[3];
    tv_ray(w, c.kp[(long)v * c.N], d);
    const double M[6] = {1.0 - d[0] * d[0], 0.0 - d[0] * d[1], 0.0 - d[0] * d[2], 1.0 - d[1] * d[1], 0.0 - d[1] * d[2], 1.0 - d[2] * d[2]};
    const double c0 = w[TV_C], c1 = w[TV_C + 1], c2 = w[TV_C + 2];
#pragma unroll
    for (int q = 0; q < 6; ++q) A[q] = A[q] + M[q];
    b[0] = b[0] + ((M[0] * c0 + M[1] * c1) + M[2] * c2);
    b[1] = b[1] + ((M[1] * c0 + M[3] * c1) + M[4] * c2);
    b[2] = b[2] + ((M[2] * c0 + M[4] * c1) + M[5] * c2);
  }
  return tv_solve(A, b, X);
}

// the Gauss-Newton step dX at X over the views of m; false: the factor failed
__device__ __forceinline__ bool tv_step(const TvCtx& c, unsigned m, const double (&X)[3], double (&dX)[3]) {
  double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int v = 0; v < c.V; ++v) {
    if (!((m >> v) & 1u)) continue;
    const double* w = c.vw + v * TV_VIEW;
    const TvRes r = tv_residual(w, c.kp[(long)v * c.N], X);
    double J[2][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      J[0][k] = (w[k] - r.ax * w[6 + k]) * r.iz;
      J[1][k] = (w[3 + k] - r.ay * w[6 + k]) * r.iz;
    }
    int q = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int e = a; e < 3; ++e) {
        H[q] = H[q] + (J[0][a] * J[0][e] + J[1][a] * J[1][e]);
        ++q;
      }
      g[a] = g[a] + (J[0][a] * r.e0 + J[1][a] * r.e1);
    }
  }
  const double rhs[3] = {0.0 - g[0], 0.0 - g[1], 0.0 - g[2]};
  return tv_solve(H, rhs, dX);
}

// grid (blocks over the points, B)
__global__ __launch_bounds__(TV_THREADS) void triangulate_views_kernel(const TvParams P) {
  __shared__ double vw[ROMA_TRACKS_MAX_VIEWS * TV_VIEW];
  __shared__ int vok[ROMA_TRACKS_MAX_VIEWS];
  __shared__ int shc[TV_WAVES][TRIANGULATE_VIEWS_STATS];
  const int b = blockIdx.y, t = threadIdx.x;
  const int V = P.V, N = P.N;
  if (t < V) {
    const long v = (long)b * V + t;
    double* w = vw + t * TV_VIEW;
    bool ok = !P.view_valid || P.view_valid[v] != 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = P.R[v * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[TV_T + i] = P.t[v * 3 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[TV_C + i] = 0.0 - ((w[i] * w[TV_T] + w[3 + i] * w[TV_T + 1]) + w[6 + i] * w[TV_T + 2]);
    const double* Kv = P.K ? P.K + v * 9 : nullptr;
    const double fx = Kv ? Kv[0] : 1.0, fy = Kv ? Kv[4] : 1.0;
    w[TV_FX] = fx;
    w[TV_FY] = fy;
    w[TV_CX] = Kv ? Kv[2] : 0.0;
    w[TV_CY] = Kv ? Kv[5] : 0.0;
    w[TV_THR] = Kv ? P.max_reproj / ((fx + fy) / 2) : P.max_reproj;
#pragma unroll
    for (int i = 0; i < TV_THR; ++i) ok = ok && isfinite(w[i]);
    vok[t] = ok ? 1 : 0;
  }
  __syncthreads();
  const bool on = !P.valid || P.valid[b] != 0;
  const int rows = !on ? 0 : (P.counts ? min(max(P.counts[b], 0), N) : N);
  const int j = blockIdx.x * TV_THREADS + t;
  int count[TRIANGULATE_VIEWS_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (j < N) {
    const double nan_ = __longlong_as_double(0x7ff8000000000000ll);
    const float nanf_ = __int_as_float(0x7fc00000);
    TvCtx c = {vw, P.kpts + (long)b * V * N + j, V, N, P.max_depth};
    unsigned flag = TRI_SKIPPED, obs = 0, m = 0;
    double X[3] = {nan_, nan_, nan_};
    float par = nanf_;
    if (j < rows) {
      count[0] = 1;
#pragma unroll 1
      for (int v = 0; v < V; ++v)
        if (vok[v] && tv_seen(c.kp[(long)v * N])) obs |= 1u << v;
      m = obs;
      flag = TRI_DEGENERATE;
      int trims = 0;
      double worst = 0.0;
      bool cheir = false;
#pragma unroll 1
      for (;;) {
        if (__popc(m) < P.min_views || !tv_midpoint(c, m, X)) break;
        int wi;
        double cost = tv_cost(c, m, X, worst, wi, cheir);
#pragma unroll 1
        for (int s = 0; s < P.gn_steps; ++s) {
          double dX[3];
          if (!tv_step(c, m, X, dX)) break;
          const double Xn[3] = {X[0] + dX[0], X[1] + dX[1], X[2] + dX[2]};
          double wn;
          int win;
          bool cn_cheir;
          const double cn = tv_cost(c, m, Xn, wn, win, cn_cheir);
          if (!(cn < cost && isfinite(cn))) break;
          X[0] = Xn[0], X[1] = Xn[1], X[2] = Xn[2];
          cost = cn, worst = wn, wi = win, cheir = cn_cheir;
        }
        if (P.trim && worst > 1.0 && __popc(m) >= 3) {
          m &= ~(1u << wi);
          ++trims;
          continue;
        }
        flag = 0;
        break;
      }
      count[6] = trims;
      if (flag) {
        X[0] = X[1] = X[2] = nan_;
        m = 0;
        count[2] = 1;
      } else {
        // parallax: the two rays in use with the smallest dot product
        double dmin = INFINITY;
        int pa = -1, pb = -1;
#pragma unroll 1
        for (int v = 0; v < V; ++v) {
          if (!((m >> v) & 1u)) continue;
          double dv[3];
          tv_ray(vw + v * TV_VIEW, c.kp[(long)v * N], dv);
#pragma unroll 1
          for (int u = v + 1; u < V; ++u) {
            if (!((m >> u) & 1u)) continue;
            double du[3];
            tv_ray(vw + u * TV_VIEW, c.kp[(long)u * N], du);
            const double dot = (dv[0] * du[0] + dv[1] * du[1]) + dv[2] * du[2];
            if (dot < dmin) {
              dmin = dot;
              pa = v;
              pb = u;
            }
          }
        }
        double pr = nan_;
        if (pa >= 0) {
          double dv[3], du[3];
          tv_ray(vw + pa * TV_VIEW, c.kp[(long)pa * N], dv);
          tv_ray(vw + pb * TV_VIEW, c.kp[(long)pb * N], du);
          const double c0 = dv[1] * du[2] - dv[2] * du[1], c1 = dv[2] * du[0] - dv[0] * du[2], c2 = dv[0] * du[1] - dv[1] * du[0];
          pr = atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), dmin) * TV_RAD_TO_DEG;
        }
        par = (float)pr;
        if (cheir) flag |= TRI_CHEIRALITY, count[3] = 1;
        if (worst > 1.0) flag |= TRI_REPROJ, count[4] = 1;
        if (!(pr >= P.min_parallax)) flag |= TRI_PARALLAX, count[5] = 1;
        if (flag == 0) count[1] = 1;
      }
    }
    const long pj = (long)b * N + j;
    P.points[pj * 3] = X[0], P.points[pj * 3 + 1] = X[1], P.points[pj * 3 + 2] = X[2];
    P.parallax[pj] = par;
    P.flags[pj] = (unsigned char)flag;
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
      const long o = ((long)b * V + v) * N + j;
      float e = nanf_;
      if ((obs >> v) & 1u) {
        const double* w = vw + v * TV_VIEW;
        const TvRes r = tv_residual(w, c.kp[(long)v * N], X);
        const double ex = w[TV_FX] * r.e0, ey = w[TV_FY] * r.e1;
        e = (float)sqrt(ex * ex + ey * ey);
      }
      P.reproj[o] = e;
      P.used[o] = (unsigned char)((m >> v) & 1u);
    }
  }
  // stats: lanes by the xor butterfly, waves in order, one integer atomic per counter
#pragma unroll
  for (int k = 0; k < TRIANGULATE_VIEWS_STATS - 1; ++k) {
    int v = count[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((t & 63) == 0) shc[t >> 6][k] = v;
  }
  __syncthreads();
  if (t < TRIANGULATE_VIEWS_STATS - 1) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < TV_WAVES; ++w) s += shc[w][t];
    if (s) atomicAdd(&P.stats[(long)b * TRIANGULATE_VIEWS_STATS + t], s);
  }
}

}  // namespace

extern "C" int roma_op_triangulate_views(const float* kpts, const double* K, const double* R, const double* t,
                                         const unsigned char* view_valid, const int* counts, const unsigned char* valid, int B, int V,
                                         int N, double max_reproj, double min_parallax, double max_depth, int min_views, int gn_steps,
                                         int trim, double* out_points, float* out_reproj, unsigned char* out_used, float* out_parallax,
                                         unsigned char* out_flags, int* out_stats, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(kpts && R && t && out_points && out_reproj && out_used && out_parallax && out_flags && out_stats,
               "triangulate_views: null pointer");
  ROMA_REQUIRE(V >= 2 && V <= ROMA_TRACKS_MAX_VIEWS, "triangulate_views: need 2 <= V <= 8 views");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "triangulate_views: B must lie in [0, 65535]");
  ROMA_REQUIRE(N >= 0 && (B == 0 || (long)V * N < (1l << 31) / B), "triangulate_views: need N >= 0 and B * V * N below 2^31");
  ROMA_REQUIRE(max_reproj >= 0 && min_parallax >= 0 && max_depth >= 0, "triangulate_views: a threshold is negative (or NaN)");
  ROMA_REQUIRE(min_views >= 2 && min_views <= V, "triangulate_views: need 2 <= min_views <= V");
  ROMA_REQUIRE(gn_steps >= 0 && gn_steps <= TRIANGULATE_VIEWS_MAX_GN, "triangulate_views: need 0 <= gn_steps <= 10");
  ROMA_REQUIRE(trim == 0 || trim == 1, "triangulate_views: trim must be 0 or 1");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(kpts) & 7) == 0, "triangulate_views: kpts must be 8-byte aligned");
  if (B == 0 || N == 0) return 0;
  ROMA_CHECK_HIP(hipMemsetAsync(out_stats, 0, (size_t)B * TRIANGULATE_VIEWS_STATS * sizeof(int), s));
  TvParams P = {reinterpret_cast<const float2*>(kpts), K, R, t, view_valid, counts, valid, V, N, min_views, gn_steps, trim,
                max_reproj, min_parallax, max_depth, out_points, out_reproj, out_used, out_parallax, out_flags, out_stats};
  ProfScope ps("triangulate_views_kernel", (double)B * (double)N * V, "B", s);
  hipLaunchKernelGGL(triangulate_views_kernel, dim3((N + TV_THREADS - 1) / TV_THREADS, B), dim3(TV_THREADS), 0, s, P);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
