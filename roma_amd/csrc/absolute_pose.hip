// Absolute pose on the device: the camera pose (R, t), x_cam = R X + t, from rows (X, x) of a 3-D point and its image - what a
// caller does with the points of triangulate / a depth map and the matches of sample_batched (visual localisation, registering
// a further image).  tools/absolute_pose_ref.py restates this file in numpy float64 expression by expression and is the oracle
// of the GPU tests.  The RANSAC is ransac.h's pipeline under CountScoring with the model policy AbsPose below: a pose is 12
// doubles (R row-major, then t) and a row the normalised 3-D point and its image point.
//
// What AbsPose adds to the shared pipeline, per pair b (counts[b] rows; later rows are never read):
//   normalise   x_n = ((u - cx) / fx, (v - cy) / fy) and the threshold divided by (fx + fy) / 2 under a camera matrix;
//               X' = s (X - c), c the centroid of the finite rows and s = 1 / their mean distance to it (f64 sums in block_sum
//               order), so that the f32 scoring works on O(1) numbers wherever the world origin is.  The pose of the normalised
//               problem is (R, t' = s (R c + t)); rows with a non-finite entry are stored as NaN (ApRows: a float4 array of the
//               points and a float2 array of the image points).  Valid: at least 4 finite rows and s finite.
//   hypothesis  one lane per hypothesis: the three rows of the sample normalised in f64, p3p: up to 4 poses
//   inlier      the f32 test z > 0, |p_xy - x_n z|^2 < thr^2 z^2
//   model_out   t = t' / s - R c.  A model needs MIN_INLIERS = 4 inliers: the three rows of a sample fit each of its solutions.
//               No refit (REFINE_ITERS = 0); the info row is {rounds, best_h, best_slot, best, valid}.
// p3p: unit bearings f_i, squared sides a2 = |X2 - X3|^2, b2 = |X1 - X3|^2, c2 = |X1 - X2|^2, cosines ca = f2.f3, cb = f1.f3,
// cg = f1.f2, depths s2 = u s1, s3 = v s1.  With A = a2 / b2, C = c2 / b2 the difference of the two conics the cosine laws give in
// (u, v) is u D(v) = N(v), N = (1 - A + C) v^2 + 2 (A - C) cb v + (C - A - 1), D = 2 (ca v - cg), and N^2 - 2 cg N D + Q D^2 = 0
// with Q = -C v^2 + 2 C cb v + (1 - C) is the quartic in v.  Its positive roots: those of p in [0, 1] and of the reversed
// polynomial (w = 1 / v) in [0, 1), by unit_roots - a fixed bisection schedule, no closed form - then AP_NEWTON Newton steps;
// per root s1 = b / sqrt(1 - 2 cb v + v^2), AP_GN Gauss-Newton steps on the cosine laws in (s1, s2, s3), and (R, t) from the
// orthonormal frames of (P2 - P1, (P2 - P1) x (P3 - P1)) in both spaces.  Slots ascend in v.
//
// abs_refine_kernel: lm_fit<AbsPoseFit> (lm_fit.h) on the normalised problem - 6 parameters (R <- exp([w]x) R, t' <- t' + dt),
// two residuals per row p_xy / z - x_n, a row with z <= 0 or a non-finite value inactive - and the mask of the final pose.
// lift_kernel: matches + depth map -> 3-D points in camera A's frame and pixel keypoints in B (depth_consistency's bilinear rule).
#include "../../include/roma_hip.h"
#include "lm_fit.h"

namespace roma {
namespace {

constexpr int ABSOLUTE_POSE_INFO = 5;  // ints per pair in roma_op_absolute_pose's out_info
constexpr int AP_SLOTS = 4;            // solutions of one P3P sample
constexpr int AP_BISECT = 48, AP_NEWTON = 3, AP_GN = 3;
constexpr double AP_DEN_EPS = 1e-9;        // |D(v)| below which u = N / D is not formed
constexpr double AP_COLLINEAR_EPS = 1e-4;  // |d12 x d13| / (|d12| |d13|) below which the 3-D sample is collinear
constexpr int AP_MIN_VALID = 4;            // finite rows below which a pair is not sampled

// ------------------------------------------------------------------------------------------------------------ normalisation
struct ApNorm {
  double c[3], s;               // X' = s (X - c)
  double fx, fy, cx, cy;        // x_n = ((u - cx) / fx, (v - cy) / fy); identity without a camera matrix
  __device__ __forceinline__ void apply(const float* X, float2 k, double (&Xn)[3], double (&xn)[2]) const {
#pragma unroll
    for (int a = 0; a < 3; ++a) Xn[a] = ((double)X[a] - c[a]) * s;
    xn[0] = ((double)k.x - cx) / fx;
    xn[1] = ((double)k.y - cy) / fy;
  }
  // whether a row (3-D point, image point), normalised or not, holds finite values only
  __device__ static bool finite(const double (&X)[3], const double (&x)[2]) {
    return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && isfinite(x[0]) && isfinite(x[1]);
  }
  // the threshold in normalised image coordinates: pixels over the mean focal length under a camera matrix
  __device__ __forceinline__ double threshold(bool camera, double thr) const { return camera ? thr / ((fx + fy) / 2) : thr; }
};

__device__ __forceinline__ ApNorm camera_norm(const double* K) {
  ApNorm nrm;
  nrm.c[0] = nrm.c[1] = nrm.c[2] = 0.0;
  nrm.s = 1.0;
  nrm.fx = K ? K[0] : 1.0;
  nrm.fy = K ? K[4] : 1.0;
  nrm.cx = K ? K[2] : 0.0;
  nrm.cy = K ? K[5] : 0.0;
  return nrm;
}

// ------------------------------------------------------------------------------------------------------------ polynomials
template <int D>
__device__ __forceinline__ double horner(const double (&c)[D + 1], double x) {
  double r = c[D];
#pragma unroll
  for (int k = D - 1; k >= 0; --k) r = r * x + c[k];
  return r;
}

template <int D>
__device__ __forceinline__ void deriv(const double (&c)[D + 1], double (&d)[D]) {
#pragma unroll
  for (int k = 1; k <= D; ++k) d[k - 1] = c[k] * (double)k;
}

// roots of c between the sorted points 0, crit, 1: one per interval with a sign change, AP_BISECT halvings; the interval's right
// end where there is none, so that `out` stays sorted
template <int D>
__device__ __forceinline__ void bisect_level(const double (&c)[D + 1], const double (&crit)[D - 1], double (&out)[D], bool (&found)[D]) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double x0 = j == 0 ? 0.0 : crit[j == 0 ? 0 : j - 1];
    const double right = j == D - 1 ? 1.0 : crit[j == D - 1 ? 0 : j];
    double x1 = right;
    const bool n0 = horner<D>(c, x0) < 0;
    const bool has = n0 != (horner<D>(c, x1) < 0);
#pragma unroll 1
    for (int it = 0; it < AP_BISECT; ++it) {
      const double mid = 0.5 * (x0 + x1);
      const bool left = (horner<D>(c, mid) < 0) == n0;
      x0 = left ? mid : x0;
      x1 = left ? x1 : mid;
    }
    out[j] = has ? 0.5 * (x0 + x1) : right;
    found[j] = has;
  }
}

// roots of the quartic c in [0, 1], ascending: the root of the linear third derivative brackets those of the second, those
// the first's, those the quartic's
__device__ __forceinline__ void unit_roots(const double (&c)[5], double (&out)[4], bool (&found)[4]) {
  double d1[4], d2[3], d3[2];
  deriv<4>(c, d1);
  deriv<3>(d1, d2);
  deriv<2>(d2, d3);
  const double r = -d3[0] / d3[1];
  const double c1[1] = {isfinite(r) && r > 0 && r < 1 ? r : 1.0};
  double c2[2], c3[3];
  bool f2[2], f3[3];
  bisect_level<2>(d2, c1, c2, f2);
  bisect_level<3>(d1, c2, c3, f3);
  bisect_level<4>(c, c3, out, found);
}

template <int NA, int NB>
__device__ __forceinline__ void polymul(const double (&a)[NA], const double (&b)[NB], double (&o)[NA + NB - 1]) {
#pragma unroll
  for (int k = 0; k < NA + NB - 1; ++k) o[k] = 0.0;
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) o[i + j] = o[i + j] + a[i] * b[j];
}

// ------------------------------------------------------------------------------------------------------------ P3P
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// the orthonormal frame e[0] = d12 / |d12|, e[2] = (d12 x d13) / |.|, e[1] = e[2] x e[0] of three points
__device__ __forceinline__ void frame3(const double* p1, const double* p2, const double* p3, double (&e)[3][3]) {
  double d12[3], d13[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d12[k] = p2[k] - p1[k]; d13[k] = p3[k] - p1[k]; }
  const double l1 = sqrt(dot3(d12, d12));
#pragma unroll
  for (int k = 0; k < 3; ++k) e[0][k] = d12[k] / l1;
  cross3(d12, d13, n);
  const double l3 = sqrt(dot3(n, n));
#pragma unroll
  for (int k = 0; k < 3; ++k) e[2][k] = n[k] / l3;
  cross3(e[2], e[0], e[1]);
}

// X [3][3] points, x [3][2] normalised image points, act: the sample is usable.  emit(slot, m): solution `slot`, m[12] = R
// row-major, then t (handed over one at a time: an array of them indexed by the running count would live in scratch); returns
// the number of solutions, ascending in v.
template <class Emit>
__device__ __forceinline__ int p3p(const double (&X)[3][3], const double (&x)[3][2], bool act, Emit emit) {
  double f[3][3];
  bool ok = act;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double nrm = sqrt((x[k][0] * x[k][0] + x[k][1] * x[k][1]) + 1.0);
    f[k][0] = x[k][0] / nrm;
    f[k][1] = x[k][1] / nrm;
    f[k][2] = 1.0 / nrm;
    ok = ok && ApNorm::finite(X[k], x[k]);
  }
  double d12[3], d13[3], d23[3], cr[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d12[k] = X[1][k] - X[0][k];
    d13[k] = X[2][k] - X[0][k];
    d23[k] = X[2][k] - X[1][k];
  }
  const double a2 = dot3(d23, d23), b2 = dot3(d13, d13), c2 = dot3(d12, d12);
  cross3(d12, d13, cr);
  ok = ok && dot3(cr, cr) > (AP_COLLINEAR_EPS * AP_COLLINEAR_EPS) * (c2 * b2);
  if (!ok) return 0;
  const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
  const double A = a2 / b2, C = c2 / b2;
  const double N[3] = {(C - A) - 1.0, (2.0 * (A - C)) * cb, (1.0 - A) + C};
  const double D[2] = {-2.0 * cg, 2.0 * ca};
  const double Q[3] = {1.0 - C, (2.0 * C) * cb, -C};
  double NN[5], ND[4], DD[3], QDD[5], p[5], pr[5], dp[4];
  polymul<3, 3>(N, N, NN);
  polymul<3, 2>(N, D, ND);
  polymul<2, 2>(D, D, DD);
  polymul<3, 3>(Q, DD, QDD);
#pragma unroll
  for (int k = 0; k < 5; ++k) p[k] = (NN[k] - (2.0 * cg) * (k < 4 ? ND[k] : 0.0)) + QDD[k];
#pragma unroll
  for (int k = 0; k < 5; ++k) pr[k] = p[4 - k];
  deriv<4>(p, dp);
  double lo[4], hi[4];
  bool flo[4], fhi[4];
  unit_roots(p, lo, flo);
  unit_roots(pr, hi, fhi);
  const double b = sqrt(b2);
  double Fw[3][3];
  frame3(X[0], X[1], X[2], Fw);
  int n = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // ascending in v: the roots in [0, 1], then 1 / w for w descending
    double v = j < 4 ? lo[j & 3] : 1.0 / hi[3 - (j & 3)];
    const bool fv = j < 4 ? flo[j & 3] : fhi[3 - (j & 3)] && hi[3 - (j & 3)] > 0 && hi[3 - (j & 3)] < 1;
#pragma unroll
    for (int it = 0; it < AP_NEWTON; ++it) {
      const double pv = horner<4>(p, v), dv = horner<3>(dp, v);
      const double v1 = v - pv / dv;
      v = isfinite(v1) && dv != 0 ? v1 : v;
    }
    const double Dv = horner<1>(D, v);
    const double u = horner<2>(N, v) / Dv;
    double s1 = b / sqrt((1.0 - (2.0 * cb) * v) + v * v);
    double s2 = u * s1, s3 = v * s1;
#pragma unroll
    for (int it = 0; it < AP_GN; ++it) {
      const double F1 = ((s2 * s2 + s3 * s3) - ((2.0 * s2) * s3) * ca) - a2;
      const double F2 = ((s1 * s1 + s3 * s3) - ((2.0 * s1) * s3) * cb) - b2;
      const double F3 = ((s1 * s1 + s2 * s2) - ((2.0 * s1) * s2) * cg) - c2;
      const double j12 = 2.0 * (s2 - s3 * ca), j13 = 2.0 * (s3 - s2 * ca);
      const double j21 = 2.0 * (s1 - s3 * cb), j23 = 2.0 * (s3 - s1 * cb);
      const double j31 = 2.0 * (s1 - s2 * cg), j32 = 2.0 * (s2 - s1 * cg);
      // Cramer's rule on [[0, j12, j13], [j21, 0, j23], [j31, j32, 0]] delta = -F
      const double det = j12 * (j23 * j31) + j13 * (j21 * j32);
      const double g1 = -F1, g2 = -F2, g3 = -F3;
      const double e1 = (j12 * (j23 * g3) + j13 * (g2 * j32)) - g1 * (j23 * j32);
      const double e2 = (j13 * (j21 * g3) + g1 * (j23 * j31)) - j13 * (g2 * j31);
      const double e3 = (j12 * (g2 * j31) + g1 * (j21 * j32)) - j12 * (j21 * g3);
      const double n1 = s1 + e1 / det, n2 = s2 + e2 / det, n3 = s3 + e3 / det;
      const bool step = isfinite(n1) && isfinite(n2) && isfinite(n3) && det != 0;
      s1 = step ? n1 : s1;
      s2 = step ? n2 : s2;
      s3 = step ? n3 : s3;
    }
    bool good = fv && fabs(Dv) >= AP_DEN_EPS && s1 > 0 && s2 > 0 && s3 > 0 && isfinite(s1) && isfinite(s2) && isfinite(s3);
    double Y[3][3], Fc[3][3], Rt[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Y[0][k] = f[0][k] * s1;
      Y[1][k] = f[1][k] * s2;
      Y[2][k] = f[2][k] * s3;
    }
    frame3(Y[0], Y[1], Y[2], Fc);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Rt[3 * r + c] = (Fc[0][r] * Fw[0][c] + Fc[1][r] * Fw[1][c]) + Fc[2][r] * Fw[2][c];
        good = good && isfinite(Rt[3 * r + c]);
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      Rt[9 + r] = Y[0][r] - ((Rt[3 * r] * X[0][0] + Rt[3 * r + 1] * X[0][1]) + Rt[3 * r + 2] * X[0][2]);
      good = good && isfinite(Rt[9 + r]);
    }
    good = good && n < AP_SLOTS;
    if (good) {
      emit(n, Rt);
      ++n;
    }
  }
  return n;
}

// ------------------------------------------------------------------------------------------------------------ model policy
struct ApIn {                   // the caller's rows: points3d [B, N, 3], kpts [B, N] pixels (normalised without a camera matrix)
  const float* X;
  const float2* k;
  __device__ ApIn at(long row) const { return {X + 3 * row, k + row}; }
};

struct ApOut {                  // R [B, 9], t [B, 3]
  double* r;
  double* t;
};

// the normalised f32 rows, two arrays (the score kernel loads one float4 and one float2 per row): (X', Y', Z', 0) and x_n, [B * N]
struct ApRows {
  struct Row { float4 X; float2 x; };
  float4* px;
  float2* pi;
  static void carve(ApRows& r, Workspace256& ws, size_t rows) {
    r.px = ws.take<float4>(rows);
    r.pi = ws.take<float2>(rows);
  }
  __device__ ApRows at(long row) const { return {px + row, pi + row}; }
  __device__ Row row(int i, int n) const {
    return {i < n ? px[i] : make_float4(NAN, NAN, NAN, NAN), i < n ? pi[i] : make_float2(NAN, NAN)};
  }
};

struct AbsPose {
  using Norm = ApNorm;
  using In = ApIn;
  using Out = ApOut;
  using Rows = ApRows;
  static constexpr int S = 3, SLOTS = AP_SLOTS, NM = 12, HYP_THREADS = 64, HYP_LANES = 1, REFINE_ITERS = 0, INFO = ABSOLUTE_POSE_INFO;
  static constexpr int MIN_INLIERS = 4;  // the three rows of a sample fit each of its solutions
  static constexpr bool SCORE_EVERY_SLOT = false;
  static_assert(INFO == INFO_CORE);

  // every thread of the workgroup: camera, centroid and scale over the finite rows (f64 sums in block_sum order), the rows;
  // one threshold (t2a == t2b)
  __device__ static bool normalise(ApIn in, int n, const double* K, float thr, double* sh, ApRows rows, ApNorm& nrm, float& t2a,
                                   float& t2b) {
    const int t = threadIdx.x;
    nrm = camera_norm(K);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int i = t; i < n; i += 256) {
      double Xn[3], xn[2];
      nrm.apply(in.X + 3 * (long)i, in.k[i], Xn, xn);
      if (ApNorm::finite(Xn, xn)) {
        s0 += Xn[0]; s1 += Xn[1]; s2 += Xn[2]; s3 += 1;
      }
    }
    const double cnt = block_sum(s3, sh);
    const double c0 = block_sum(s0, sh) / cnt, c1 = block_sum(s1, sh) / cnt, c2 = block_sum(s2, sh) / cnt;
    double dsum = 0;
    for (int i = t; i < n; i += 256) {
      double Xn[3], xn[2];
      nrm.apply(in.X + 3 * (long)i, in.k[i], Xn, xn);
      if (ApNorm::finite(Xn, xn)) {
        const double d0 = Xn[0] - c0, d1 = Xn[1] - c1, d2 = Xn[2] - c2;
        dsum += sqrt((d0 * d0 + d1 * d1) + d2 * d2);
      }
    }
    const double mean = block_sum(dsum, sh) / cnt;
    nrm.c[0] = c0; nrm.c[1] = c1; nrm.c[2] = c2;
    nrm.s = mean > 0 ? 1.0 / mean : INFINITY;
    for (int i = t; i < n; i += 256) {
      double Xn[3], xn[2];
      nrm.apply(in.X + 3 * (long)i, in.k[i], Xn, xn);
      const bool fin = ApNorm::finite(Xn, xn);
      rows.px[i] = fin ? make_float4((float)Xn[0], (float)Xn[1], (float)Xn[2], 0.f) : make_float4(NAN, NAN, NAN, NAN);
      rows.pi[i] = fin ? make_float2((float)xn[0], (float)xn[1]) : make_float2(NAN, NAN);
    }
    const double tn = nrm.threshold(K != nullptr, (double)thr);
    t2a = t2b = (float)(tn * tn);
    return cnt >= AP_MIN_VALID && isfinite(nrm.s);
  }

  // one lane per hypothesis: a row that is not finite makes p3p return no model
  __device__ static void hypothesis(ApIn in, const int (&idx)[3], bool act, const ApNorm& nrm, int g, int, const Slots& sl) {
    double X[3][3], x[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long row = act ? idx[k] : 0;
      nrm.apply(in.X + 3 * row, in.k[row], X[k], x[k]);
    }
    sl.n[g] = p3p(X, x, act, [&](int s, const double (&m)[12]) { store_model<12>(m, (long)g * AP_SLOTS + s, sl); });
  }

  // z > 0 and |p_xy - x_n z|^2 < thr^2 z^2 with p = R X' + t'; false for a NaN row
  __device__ static bool inlier(const float* m, ApRows::Row r, float thr2, float) {
    const float4 X = r.X;
    const float2 x = r.x;
    const float px = fmaf(m[0], X.x, fmaf(m[1], X.y, fmaf(m[2], X.z, m[9])));
    const float py = fmaf(m[3], X.x, fmaf(m[4], X.y, fmaf(m[5], X.z, m[10])));
    const float z = fmaf(m[6], X.x, fmaf(m[7], X.y, fmaf(m[8], X.z, m[11])));
    const float ex = fmaf(-x.x, z, px), ey = fmaf(-x.y, z, py);
    return z > 0.f && fmaf(ex, ex, ey * ey) < thr2 * (z * z);
  }

  // the pose of the caller's problem: t = t' / s - R c
  __device__ static void model_out(const PairState<AbsPose>& P, bool good, ApOut out, int b) {
    const double* m = P.cur;
    const double* c = P.nrm.c;
    for (int k = 0; k < 9; ++k) out.r[(long)b * 9 + k] = good ? m[k] : 0.0;
    for (int r = 0; r < 3; ++r)
      out.t[(long)b * 3 + r] = good ? m[9 + r] / P.nrm.s - ((m[3 * r] * c[0] + m[3 * r + 1] * c[1]) + m[3 * r + 2] * c[2]) : 0.0;
  }
};

// ------------------------------------------------------------------------------------------------------------ the solver alone
__global__ __launch_bounds__(64) void ap_minimal_kernel(const double* __restrict__ X, const double* __restrict__ x, int S,
                                                        double* __restrict__ out_r, double* __restrict__ out_t, int* __restrict__ out_n) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= S) return;
  double Xs[3][3], xs[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int a = 0; a < 3; ++a) Xs[k][a] = X[(long)g * 9 + 3 * k + a];
    xs[k][0] = x[(long)g * 6 + 2 * k];
    xs[k][1] = x[(long)g * 6 + 2 * k + 1];
  }
  const int nm = p3p(Xs, xs, true, [&](int s, const double (&m)[12]) {
    const long slot = (long)g * AP_SLOTS + s;
#pragma unroll
    for (int k = 0; k < 9; ++k) out_r[slot * 9 + k] = m[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_t[slot * 3 + k] = m[9 + k];
  });
  out_n[g] = nm;
  for (int s = nm; s < AP_SLOTS; ++s) {
    const long slot = (long)g * AP_SLOTS + s;
    for (int k = 0; k < 9; ++k) out_r[slot * 9 + k] = 0.0;
    for (int k = 0; k < 3; ++k) out_t[slot * 3 + k] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------------------ refinement
struct AbsPoseFit {
  static constexpr int NP = 6, NR = 2, MIN_ROWS = 3;
  struct State { double R[9], t[3]; };
  using Prep = ApNorm;
  struct Aux { double R[9], t[3]; };
  struct Point { double X[3], x[2]; };
  struct Row { double q[3], iz, ax, ay; };

  // row i of the 3-D points (three floats each, behind ka) and of the image points, normalised in f64
  __device__ static Point row(const Prep& q, const float2* ka, const float2* kb, int i) {
    Point w;
    q.apply(reinterpret_cast<const float*>(ka) + 3 * (long)i, kb[i], w.X, w.x);
    return w;
  }

  __device__ static void aux(const State& s, const Prep&, Aux& ax) {
#pragma unroll
    for (int k = 0; k < 9; ++k) ax.R[k] = s.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ax.t[k] = s.t[k];
  }

  // p = R X' + t', e = p_xy / z - x_n; NaN (never active) unless z > 0
  __device__ static double residual(const Aux& ax, const Point& z, Row& w, double (&e)[NR]) {
    double p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w.q[i] = (ax.R[3 * i] * z.X[0] + ax.R[3 * i + 1] * z.X[1]) + ax.R[3 * i + 2] * z.X[2];
      p[i] = w.q[i] + ax.t[i];
    }
    w.iz = 1.0 / p[2];
    w.ax = p[0] * w.iz;
    w.ay = p[1] * w.iz;
    e[0] = w.ax - z.x[0];
    e[1] = w.ay - z.x[1];
    return p[2] > 0 ? e[0] * e[0] + e[1] * e[1] : NAN;
  }

  // de = ((dp_x - a_x dp_z) / z, (dp_y - a_y dp_z) / z) with dp = e_k x q for the rotation about e_k and e_k for dt_k
  __device__ static void jacobian(const State&, const Aux&, const Point&, const Row& w, const double (&)[NR], double (&J)[NR][NP]) {
    const double* q = w.q;
    const double iz = w.iz, ax = w.ax, ay = w.ay;
    J[0][0] = (0.0 - ax * q[1]) * iz;
    J[0][1] = (q[2] - ax * (-q[0])) * iz;
    J[0][2] = ((-q[1]) - ax * 0.0) * iz;
    J[1][0] = ((-q[2]) - ay * q[1]) * iz;
    J[1][1] = (0.0 - ay * (-q[0])) * iz;
    J[1][2] = (q[0] - ay * 0.0) * iz;
    J[0][3] = iz;
    J[0][4] = 0.0;
    J[0][5] = (0.0 - ax) * iz;
    J[1][3] = 0.0;
    J[1][4] = iz;
    J[1][5] = (0.0 - ay) * iz;
  }

  __device__ static void apply(const State& s, const double (&d)[NP], State& o) {
    double E[9];
    lm_rodrigues(d[0], d[1], d[2], E);
    mat3(E, s.R, o.R);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.t[k] = s.t[k] + d[3 + k];
  }
};

__global__ __launch_bounds__(LM_THREADS) void abs_refine_kernel(const double* __restrict__ R_in, const double* __restrict__ t_in,
                                                                const float* __restrict__ pts3, const float2* __restrict__ kpts,
                                                                const int* __restrict__ counts, const unsigned char* __restrict__ valid,
                                                                const double* __restrict__ K, int N, double thr, int max_steps,
                                                                double* __restrict__ out_R, double* __restrict__ out_t,
                                                                unsigned char* __restrict__ mask, int* __restrict__ out_info) {
  __shared__ double shn[LM_WAVES * lm_sums(AbsPoseFit::NP)];
  __shared__ double sh[LM_WAVES];
  __shared__ int shc[LM_WAVES];
  const int b = blockIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  const float2* ka = reinterpret_cast<const float2*>(pts3 + (long)b * N * 3);  // read by AbsPoseFit::row alone
  const float2* kb = kpts + (long)b * N;
  // the normalisation of AbsPose::normalise (the waves' sums in lm_reduce's order)
  ApNorm nrm = camera_norm(K ? K + (long)b * 9 : nullptr);
  const double thr_n = nrm.threshold(K != nullptr, thr);
  double sum[3] = {0.0, 0.0, 0.0};
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    const AbsPoseFit::Point w = AbsPoseFit::row(nrm, ka, kb, i);
    if (ApNorm::finite(w.X, w.x)) {
      sum[0] += w.X[0]; sum[1] += w.X[1]; sum[2] += w.X[2];
      ++cnt;
    }
  }
  lm_reduce(sum, cnt, shn, shc);
  const double c0 = sum[0] / cnt, c1 = sum[1] / cnt, c2 = sum[2] / cnt;
  double ds[1] = {0.0};
  int cnt2 = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    const AbsPoseFit::Point w = AbsPoseFit::row(nrm, ka, kb, i);
    if (ApNorm::finite(w.X, w.x)) {
      const double d0 = w.X[0] - c0, d1 = w.X[1] - c1, d2 = w.X[2] - c2;
      ds[0] += sqrt((d0 * d0 + d1 * d1) + d2 * d2);
      ++cnt2;
    }
  }
  lm_reduce(ds, cnt2, sh, shc);
  const double mean = ds[0] / cnt;
  nrm.c[0] = c0; nrm.c[1] = c1; nrm.c[2] = c2;
  nrm.s = mean > 0 ? 1.0 / mean : INFINITY;

  AbsPoseFit::State S;
  double tin[3];
  bool ok = (!valid || valid[b]) && n >= AbsPoseFit::MIN_ROWS && cnt >= AP_MIN_VALID && isfinite(nrm.s);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    S.R[k] = R_in[(long)b * 9 + k];
    ok = ok && isfinite(S.R[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    tin[k] = t_in[(long)b * 3 + k];
    ok = ok && isfinite(tin[k]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) S.t[r] = nrm.s * (((S.R[3 * r] * c0 + S.R[3 * r + 1] * c1) + S.R[3 * r + 2] * c2) + tin[r]);
  LmResult fit = {0, 0, 0, NAN, NAN};
  // uniform over the workgroup, like every branch of the loop: all threads hold the same values
  if (ok) fit = lm_fit<AbsPoseFit>(S, nrm, ka, kb, n, thr_n * thr_n, max_steps, shn, sh, shc);
  if (threadIdx.x == 0) {
    // without an accepted step the input comes back untouched
    for (int k = 0; k < 9; ++k) out_R[(long)b * 9 + k] = fit.steps ? S.R[k] : R_in[(long)b * 9 + k];
    for (int r = 0; r < 3; ++r)
      out_t[(long)b * 3 + r] = fit.steps ? S.t[r] / nrm.s - ((S.R[3 * r] * c0 + S.R[3 * r + 1] * c1) + S.R[3 * r + 2] * c2) : tin[r];
    out_info[b * 4] = fit.steps;
    out_info[b * 4 + 1] = fit.evals;
    out_info[b * 4 + 2] = fit.nact;
    out_info[b * 4 + 3] = ok ? 1 : 0;
  }
  // the rows active under the pose returned
  AbsPoseFit::Aux ax;
  AbsPoseFit::aux(S, nrm, ax);
  for (int i = threadIdx.x; i < N; i += LM_THREADS) {
    bool in = false;
    if (ok && i < n) {
      AbsPoseFit::Row w;
      double e[2];
      in = AbsPoseFit::residual(ax, AbsPoseFit::row(nrm, ka, kb, i), w, e) < thr_n * thr_n;
    }
    mask[(long)b * N + i] = in ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------------------ lifting
// grid (ceil(N / 256), B): f64 arithmetic, rounded once at the store
__global__ __launch_bounds__(256) void lift_kernel(const float* __restrict__ matches, const float* __restrict__ depth,
                                                   const double* __restrict__ K, int N, int H, int W, int H_B, int W_B,
                                                   float* __restrict__ points, float* __restrict__ kpts_b) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const long row = (long)b * N + i;
  const double m0 = matches[row * 4], m1 = matches[row * 4 + 1], m2 = matches[row * 4 + 2], m3 = matches[row * 4 + 3];
  const double* Kb = K + (long)b * 9;
  const double gw = (double)W, gh = (double)H;
  const double px = (gw / 2) * (m0 + 1.0), py = (gh / 2) * (m1 + 1.0);
  const double gx = px - 0.5, gy = py - 0.5;
  const double fx0 = floor(gx), fy0 = floor(gy);
  double X = NAN, Y = NAN, Z = NAN;
  // the four neighbours lie inside the map (NaN fails every comparison)
  if (fx0 >= 0.0 && fx0 + 1.0 <= gw - 1.0 && fy0 >= 0.0 && fy0 + 1.0 <= gh - 1.0) {
    const float* d = depth + ((long)b * H + (long)fy0) * W + (long)fx0;
    const double d00 = d[0], d01 = d[1], d10 = d[W], d11 = d[W + 1];
    if (isfinite(d00) && isfinite(d01) && isfinite(d10) && isfinite(d11) && d00 > 0 && d01 > 0 && d10 > 0 && d11 > 0) {
      const double ax = gx - fx0, ay = gy - fy0;
      Z = (d00 * (1.0 - ax) + d01 * ax) * (1.0 - ay) + (d10 * (1.0 - ax) + d11 * ax) * ay;
      X = (px - Kb[2]) / Kb[0] * Z;
      Y = (py - Kb[5]) / Kb[4] * Z;
    }
  }
  points[row * 3] = (float)X;
  points[row * 3 + 1] = (float)Y;
  points[row * 3 + 2] = (float)Z;
  kpts_b[row * 2] = (float)(((double)W_B / 2) * (m2 + 1.0));
  kpts_b[row * 2 + 1] = (float)(((double)H_B / 2) * (m3 + 1.0));
}

}  // namespace

extern "C" long roma_op_absolute_pose_workspace(int B, int N) { return workspace_bytes<AbsPose, CountScoring>(B, N); }

extern "C" int roma_op_absolute_pose(const float* points3d, const float* kpts, const int* counts, const unsigned long long* seeds,
                                     const double* K, int B, int N, float thr, double conf, int max_iters, double* out_r, double* out_t,
                                     unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* ws, long workspace_bytes,
                                     void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  if (check_args<CountScoring>("absolute_pose", "conf", points3d && kpts && seeds && out_r && out_t && out_mask && out_ok && out_info && ws,
                               B, N, thr, conf, max_iters, 0, ws_bytes, (size_t)roma_op_absolute_pose_workspace(B, N)))
    return -1;
  return ransac_run<AbsPose, CountScoring>({points3d, reinterpret_cast<const float2*>(kpts)}, counts, seeds, K, B, N, thr, conf,
                                           max_iters, 0, {out_r, out_t}, out_mask, out_ok, out_info, nullptr, ws, s);
}

extern "C" int roma_op_absolute_pose_minimal(const double* X, const double* x, int S, double* out_r, double* out_t, int* out_n,
                                             void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(X && x && out_r && out_t && out_n, "absolute_pose_minimal: null pointer");
  ROMA_REQUIRE(S > 0 && S <= (1 << 24), "absolute_pose_minimal: need 0 < S <= 2^24");
  hipLaunchKernelGGL(ap_minimal_kernel, dim3((S + 63) / 64), dim3(64), 0, s, X, x, S, out_r, out_t, out_n);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_refine_absolute_pose(const double* R_, const double* t, const float* points3d, const float* kpts, const int* counts,
                                            const unsigned char* valid, const double* K, int B, int N, double thr, int max_steps,
                                            double* out_r, double* out_t, unsigned char* out_mask, int* out_info, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(R_ && t && points3d && kpts && out_r && out_t && out_mask && out_info, "refine_absolute_pose: null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16),
               "refine_absolute_pose: need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(thr > 0 && isfinite(thr), "refine_absolute_pose: threshold must be positive and finite");
  ROMA_REQUIRE(max_steps >= 0 && max_steps <= (1 << 16), "refine_absolute_pose: need 0 <= max_steps <= 65536");
  hipLaunchKernelGGL(abs_refine_kernel, dim3(B), dim3(LM_THREADS), 0, s, R_, t, points3d, reinterpret_cast<const float2*>(kpts), counts,
                     valid, K, N, thr, max_steps, out_r, out_t, out_mask, out_info);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_lift_matches(const float* matches, const float* depth, const double* K, int B, int N, int H, int W, int H_B, int W_B,
                                    float* out_points, float* out_kpts, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(matches && depth && K && out_points && out_kpts, "lift_matches: null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16), "lift_matches: need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(H > 0 && W > 0 && H_B > 0 && W_B > 0 && (long)B * H * W < (1l << 40), "lift_matches: need positive image sizes");
  hipLaunchKernelGGL(lift_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, matches, depth, K, N, H, W, H_B, W_B, out_points, out_kpts);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
