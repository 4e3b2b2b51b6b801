// Registration of 3-D point sets on the device: the similarity (or rigid) transform y ~ s R x + t between rows (x, y) of
// corresponding points - what joins two reconstructions that share views (each lives in a gauge of its own: origin at its view
// 0, scale from its seed pair) and what a trajectory or a cloud is scored against ground truth with.  tools/registration_ref.py
// restates this file in numpy float64 expression by expression and is the oracle of the GPU tests.  The RANSAC is ransac.h's
// pipeline under CountScoring with the model policy Sim3 below: a model is 12 doubles (A = s R row-major, then t) and a row the
// two normalised points.
//
// One closed form, sim3_from_moments, serves the minimal solver, the refinement and the trajectory error.  From the count n, the
// centroids xb, yb, sxx = sum |x - xb|^2 and the cross-covariance C = sum (y - yb)(x - xb)^T:
//   rotation     Horn's 4 x 4 symmetric matrix of C; its largest eigenvector by SIM3_SWEEPS sweeps of cyclic two-sided Jacobi over
//                the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), in registers, a fixed schedule with no convergence test; the unit
//                quaternion gives R: always a proper rotation, a mirrored set has no reflection case to handle
//   scale        Umeyama's s = sum (y - yb) . R (x - xb) / sxx = <R, C> / sxx, the minimiser over s of sum |s R x' - y'|^2 - the
//                one-sided residual that the threshold tests (Horn's symmetric scale minimises another cost); 1 when !with_scale
//   translation  t = yb - s R xb
//   no model     n < 3; s not finite or s <= 0; the two largest eigenvalues closer than SIM3_GAP_EPS times the largest (their gap is
//                twice the second singular value of C: the rotation about a line of points is free).  A three-point sample is
//                refused before that by AP_COLLINEAR_EPS's rule in either set: |d12 x d13| < 1e-4 |d12| |d13|.
//
// What Sim3 adds to the shared pipeline, per problem b (counts[b] rows; later rows are never read):
//   normalise   x' = sx (x - cx), y' = sy (y - cy): the centroids over the rows finite in both sets, sx, sy = 1 / the mean distance
//               to them (f64 sums in block_sum order); !with_scale: sy = sx, so that a rigid fit stays rigid; the threshold, a
//               distance in the destination's units, times sy.  Rows with a non-finite entry are stored as NaN (SimRows: two
//               float4 arrays).  Valid: at least 4 finite rows and both scales finite.
//   hypothesis  one lane per hypothesis: the three rows normalised in f64, their moments, sim3_from_moments
//   inlier      the f32 test |A x' + t' - y'|^2 < thr'^2
//   model_out   s = sqrt(|A'|_F^2 / 3) sx / sy (1 when !with_scale), R = A' / sqrt(|A'|_F^2 / 3), t = cy + t' / sy - s R cx.
//               MIN_INLIERS = 4: the three rows of a sample fit its model.  No refit; info = {rounds, best_h, best_slot, best, valid}.
//
// sim3_refine_kernel: one workgroup per problem on the normalised problem, f64 rows.  A step is the closed form on the rows
// active under the current model (r^2 < thr^2; without a start: every finite row), kept only if the truncated cost
// sum min(r^2, thr^2) over the finite rows is strictly lower; else the loop stops.  Two passes per step: the cost, the count and the
// sums of the active rows of a model in one, their centred moments in the other; every sum in lm_reduce's order.
// sim3_trajectory_kernel: the same passes on the camera centres -R^T t of two paths, no truncation, then the per-view errors.
// sim3_apply_*: X' = s R X + t on points, R_c' = R_c R^T, t_c' = s t_c - R_c' t on cameras (they see the moved points as before,
// the scene scaled by s).  depth_rows_kernel: the rows of one image that two reconstructions share, lift_kernel's pixel centres.
#include "../../include/roma_hip_registration.h"
#include "lm_fit.h"

#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int ALIGN_POINTS_INFO = 5;         // ints per problem in roma_op_align_points' out_info
constexpr int SIM3_SWEEPS = 6;               // Jacobi sweeps over the six pairs of Horn's matrix
constexpr double SIM3_COLLINEAR_EPS = 1e-4;  // AP_COLLINEAR_EPS's rule on a three-point sample, either set
constexpr double SIM3_GAP_EPS = 1e-8;        // (lambda_1 - lambda_2) / lambda_1 of Horn's matrix below which the rotation is free
constexpr int SIM3_MIN_VALID = 4;            // finite rows below which a problem is not sampled
constexpr int SIM3_MIN_ROWS = 3;             // rows below which the closed form has no model

// ------------------------------------------------------------------------------------------------------------ the closed form
struct Sim3Model {
  double s, R[9], t[3];
};

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// |d12 x d13|^2 > eps^2 |d12|^2 |d13|^2
__device__ __forceinline__ bool triangle_ok(const double* p1, const double* p2, const double* p3) {
  double d12[3], d13[3], cr[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d12[k] = p2[k] - p1[k]; d13[k] = p3[k] - p1[k]; }
  cr[0] = d12[1] * d13[2] - d12[2] * d13[1];
  cr[1] = d12[2] * d13[0] - d12[0] * d13[2];
  cr[2] = d12[0] * d13[1] - d12[1] * d13[0];
  return dot3(cr, cr) > (SIM3_COLLINEAR_EPS * SIM3_COLLINEAR_EPS) * (dot3(d12, d12) * dot3(d13, d13));
}

// one two-sided Jacobi rotation of the symmetric a in the (P, Q) plane, accumulated into the columns of v
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
  const double th = (aqq - app) / (2.0 * apq);
  const double tt = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
  const double t = apq != 0.0 ? tt : 0.0;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] = app - t * apq;
  a[Q][Q] = aqq + t * apq;
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k != P && k != Q) {
      const double akp = a[k][P], akq = a[k][Q];
      const double np_ = c * akp - s * akq, nq = s * akp + c * akq;
      a[k][P] = np_; a[P][k] = np_;
      a[k][Q] = nq; a[Q][k] = nq;
    }
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
}

// C row-major: C[3 a + b] = sum (y - yb)_a (x - xb)_b
__device__ __forceinline__ bool sim3_from_moments(double n, const double (&xb)[3], const double (&yb)[3], double sxx,
                                                  const double (&C)[9], bool with_scale, Sim3Model& m) {
  // Horn: S_ab = sum x'_a y'_b = C[3 b + a]
  const double Sxx = C[0], Sxy = C[3], Sxz = C[6], Syx = C[1], Syy = C[4], Syz = C[7], Szx = C[2], Szy = C[5], Szz = C[8];
  double a[4][4], v[4][4];
  a[0][0] = (Sxx + Syy) + Szz;
  a[1][1] = (Sxx - Syy) - Szz;
  a[2][2] = (Syy - Sxx) - Szz;
  a[3][3] = (Szz - Sxx) - Syy;
  a[0][1] = a[1][0] = Syz - Szy;
  a[0][2] = a[2][0] = Szx - Sxz;
  a[0][3] = a[3][0] = Sxy - Syx;
  a[1][2] = a[2][1] = Sxy + Syx;
  a[1][3] = a[3][1] = Szx + Sxz;
  a[2][3] = a[3][2] = Syz + Szy;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < SIM3_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<0, 3>(a, v);
    jacobi_rotate<1, 2>(a, v);
    jacobi_rotate<1, 3>(a, v);
    jacobi_rotate<2, 3>(a, v);
  }
  // the largest eigenvalue (the first on ties), the second largest, the eigenvector: selects, no indexing
  int k = 0;
  double lam = a[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool up = a[j][j] > lam;
    lam = up ? a[j][j] : lam;
    k = up ? j : k;
  }
  double lam2 = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) lam2 = (j != k && a[j][j] > lam2) ? a[j][j] : lam2;
  double q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = k == 0 ? v[i][0] : k == 1 ? v[i][1] : k == 2 ? v[i][2] : v[i][3];
  const double qn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
  m.R[0] = ((w * w + x * x) - y * y) - z * z;
  m.R[1] = 2.0 * (x * y - w * z);
  m.R[2] = 2.0 * (x * z + w * y);
  m.R[3] = 2.0 * (x * y + w * z);
  m.R[4] = ((w * w - x * x) + y * y) - z * z;
  m.R[5] = 2.0 * (y * z - w * x);
  m.R[6] = 2.0 * (x * z - w * y);
  m.R[7] = 2.0 * (y * z + w * x);
  m.R[8] = ((w * w - x * x) - y * y) + z * z;
  const double num = (dot3(m.R, C) + dot3(m.R + 3, C + 3)) + dot3(m.R + 6, C + 6);
  m.s = with_scale ? num / sxx : 1.0;
  bool ok = n >= (double)SIM3_MIN_ROWS && isfinite(m.s) && m.s > 0.0 && (lam - lam2) > SIM3_GAP_EPS * lam;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    m.t[r] = yb[r] - m.s * dot3(m.R + 3 * r, xb);
    ok = ok && isfinite(m.t[r]);
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) ok = ok && isfinite(m.R[e]);
  return ok;
}

// the model of three rows x [3][3], y [3][3]; act: the sample is usable
__device__ __forceinline__ bool sim3_minimal(const double (&x)[3][3], const double (&y)[3][3], bool act, bool with_scale, Sim3Model& m) {
  bool ok = act;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && isfinite(x[k][c]) && isfinite(y[k][c]);
  ok = ok && triangle_ok(x[0], x[1], x[2]) && triangle_ok(y[0], y[1], y[2]);
  double xb[3], yb[3], C[9], sxx = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xb[c] = ((x[0][c] + x[1][c]) + x[2][c]) / 3.0;
    yb[c] = ((y[0][c] + y[1][c]) + y[2][c]) / 3.0;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) C[e] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double dx[3], dy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { dx[c] = x[k][c] - xb[c]; dy[c] = y[k][c] - yb[c]; }
    sxx = sxx + dot3(dx, dx);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) C[3 * a + c] = C[3 * a + c] + dy[a] * dx[c];
  }
  const bool found = sim3_from_moments(3.0, xb, yb, sxx, C, with_scale, m);
  return ok && found;
}

// ------------------------------------------------------------------------------------------------------------ normalisation
struct SimNorm {
  double cx[3], cy[3], sx, sy;  // x' = sx (x - cx), y' = sy (y - cy)
  int with_scale;
  __device__ __forceinline__ void apply(const float* x, const float* y, double (&xn)[3], double (&yn)[3]) const {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      xn[a] = ((double)x[a] - cx[a]) * sx;
      yn[a] = ((double)y[a] - cy[a]) * sy;
    }
  }
  __device__ static bool finite(const double (&x)[3], const double (&y)[3]) {
    return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]);
  }
  __device__ static SimNorm identity(int with_scale) {
    SimNorm n;
#pragma unroll
    for (int a = 0; a < 3; ++a) { n.cx[a] = 0.0; n.cy[a] = 0.0; }
    n.sx = 1.0;
    n.sy = 1.0;
    n.with_scale = with_scale;
    return n;
  }
  // centroids c (six sums over `cnt` rows) and mean distances into the scales
  __device__ __forceinline__ void set(const double* c, double mx, double my) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { cx[a] = c[a]; cy[a] = c[3 + a]; }
    sx = mx > 0 ? 1.0 / mx : INFINITY;
    sy = with_scale ? (my > 0 ? 1.0 / my : INFINITY) : sx;
  }
  // the model of the caller's problem from that of the normalised one
  __device__ __forceinline__ void denormalise(double sn, const double* Rn, const double* tn, double& s, double* t) const {
    s = with_scale ? sn * (sx / sy) : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = (cy[r] + tn[r] / sy) - s * dot3(Rn + 3 * r, cx);
  }
};

// ------------------------------------------------------------------------------------------------------------ model policy
struct SimIn {                  // the caller's rows: src, dst [B, N, 3]
  const float* x;
  const float* y;
  int with_scale;
  __device__ SimIn at(long row) const { return {x + 3 * row, y + 3 * row, with_scale}; }
};

struct SimOut {                 // scale [B], R [B, 9], t [B, 3]
  double* s;
  double* r;
  double* t;
};

struct SimRows {                // the normalised f32 rows: (x', 0) and (y', 0), [B * N] each
  struct Row { float4 x; float4 y; };
  float4* px;
  float4* py;
  static void carve(SimRows& r, Workspace256& ws, size_t rows) {
    r.px = ws.take<float4>(rows);
    r.py = ws.take<float4>(rows);
  }
  __device__ SimRows at(long row) const { return {px + row, py + row}; }
  __device__ Row row(int i, int n) const {
    const float4 nan = make_float4(NAN, NAN, NAN, NAN);
    return {i < n ? px[i] : nan, i < n ? py[i] : nan};
  }
};

struct Sim3 {
  using Norm = SimNorm;
  using In = SimIn;
  using Out = SimOut;
  using Rows = SimRows;
  static constexpr int S = 3, SLOTS = 1, NM = 12, HYP_THREADS = 64, HYP_LANES = 1, REFINE_ITERS = 0, INFO = ALIGN_POINTS_INFO;
  static constexpr int MIN_INLIERS = 4;  // the three rows of a sample fit its model
  static constexpr bool SCORE_EVERY_SLOT = false;
  static_assert(INFO == INFO_CORE);

  // every thread of the workgroup: centroids and scales over the rows finite in both sets (f64 sums in block_sum order), the rows
  __device__ static bool normalise(SimIn in, int n, const double*, float thr, double* sh, SimRows rows, SimNorm& nrm, float& t2a,
                                   float& t2b) {
    const int t = threadIdx.x;
    nrm = SimNorm::identity(in.with_scale);
    double s[6] = {0, 0, 0, 0, 0, 0}, sc = 0;
    for (int i = t; i < n; i += 256) {
      double x[3], y[3];
      nrm.apply(in.x + 3 * (long)i, in.y + 3 * (long)i, x, y);
      if (SimNorm::finite(x, y)) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s[a] += x[a]; s[3 + a] += y[a]; }
        sc += 1;
      }
    }
    const double cnt = block_sum(sc, sh);
    double c[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) c[a] = block_sum(s[a], sh) / cnt;
    double dx = 0, dy = 0;
    for (int i = t; i < n; i += 256) {
      double x[3], y[3];
      nrm.apply(in.x + 3 * (long)i, in.y + 3 * (long)i, x, y);
      if (SimNorm::finite(x, y)) {
        const double a0 = x[0] - c[0], a1 = x[1] - c[1], a2 = x[2] - c[2];
        const double b0 = y[0] - c[3], b1 = y[1] - c[4], b2 = y[2] - c[5];
        dx += sqrt((a0 * a0 + a1 * a1) + a2 * a2);
        dy += sqrt((b0 * b0 + b1 * b1) + b2 * b2);
      }
    }
    const double mx = block_sum(dx, sh) / cnt, my = block_sum(dy, sh) / cnt;
    nrm.set(c, mx, my);
    const float4 nan = make_float4(NAN, NAN, NAN, NAN);
    for (int i = t; i < n; i += 256) {
      const float* px = in.x + 3 * (long)i;
      const float* py = in.y + 3 * (long)i;
      double x[3], y[3];
      nrm.apply(px, py, x, y);
      const bool fin = isfinite(px[0]) && isfinite(px[1]) && isfinite(px[2]) && isfinite(py[0]) && isfinite(py[1]) && isfinite(py[2]);
      rows.px[i] = fin ? make_float4((float)x[0], (float)x[1], (float)x[2], 0.f) : nan;
      rows.py[i] = fin ? make_float4((float)y[0], (float)y[1], (float)y[2], 0.f) : nan;
    }
    const double tn = (double)thr * nrm.sy;
    t2a = t2b = (float)(tn * tn);
    return cnt >= SIM3_MIN_VALID && isfinite(nrm.sx) && isfinite(nrm.sy);
  }

  // one lane per hypothesis: a row that is not finite makes sim3_minimal return no model
  __device__ static void hypothesis(SimIn in, const int (&idx)[3], bool act, const SimNorm& nrm, int g, int, const Slots& sl) {
    double x[3][3], y[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long row = act ? idx[k] : 0;
      nrm.apply(in.x + 3 * row, in.y + 3 * row, x[k], y[k]);
    }
    Sim3Model m;
    const bool found = sim3_minimal(x, y, act, nrm.with_scale != 0, m);
    if (found) {
      double A[12];
#pragma unroll
      for (int e = 0; e < 9; ++e) A[e] = m.s * m.R[e];
#pragma unroll
      for (int r = 0; r < 3; ++r) A[9 + r] = m.t[r];
      store_model<12>(A, (long)g, sl);
    }
    sl.n[g] = found ? 1 : 0;
  }

  // |A x' + t' - y'|^2 < thr^2; false for a NaN row
  __device__ static bool inlier(const float* m, SimRows::Row r, float thr2, float) {
    const float4 X = r.x, Y = r.y;
    const float ex = fmaf(m[0], X.x, fmaf(m[1], X.y, fmaf(m[2], X.z, m[9]))) - Y.x;
    const float ey = fmaf(m[3], X.x, fmaf(m[4], X.y, fmaf(m[5], X.z, m[10]))) - Y.y;
    const float ez = fmaf(m[6], X.x, fmaf(m[7], X.y, fmaf(m[8], X.z, m[11]))) - Y.z;
    return fmaf(ex, ex, fmaf(ey, ey, ez * ez)) < thr2;
  }

  __device__ static void model_out(const PairState<Sim3>& P, bool good, SimOut out, int b) {
    const double* A = P.cur;
    double f2 = 0.0;
    for (int e = 0; e < 9; ++e) f2 = f2 + A[e] * A[e];
    const double sn = P.nrm.with_scale ? sqrt(f2 / 3.0) : 1.0;
    double Rn[9], s, t[3];
    for (int e = 0; e < 9; ++e) Rn[e] = A[e] / sn;
    P.nrm.denormalise(sn, Rn, A + 9, s, t);
    out.s[b] = good ? s : 0.0;
    for (int e = 0; e < 9; ++e) out.r[(long)b * 9 + e] = good ? Rn[e] : 0.0;
    for (int r = 0; r < 3; ++r) out.t[(long)b * 3 + r] = good ? t[r] : 0.0;
  }
};

// ------------------------------------------------------------------------------------------------------------ the solver alone
__global__ __launch_bounds__(64) void sim3_minimal_kernel(const double* __restrict__ X, const double* __restrict__ Y, int S, int with_scale,
                                                          double* __restrict__ out_s, double* __restrict__ out_r,
                                                          double* __restrict__ out_t, int* __restrict__ out_n) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= S) return;
  double x[3][3], y[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      x[k][a] = X[(long)g * 9 + 3 * k + a];
      y[k][a] = Y[(long)g * 9 + 3 * k + a];
    }
  Sim3Model m;
  const bool found = sim3_minimal(x, y, true, with_scale != 0, m);
  out_s[g] = found ? m.s : 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) out_r[(long)g * 9 + e] = found ? m.R[e] : 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) out_t[(long)g * 3 + r] = found ? m.t[r] : 0.0;
  out_n[g] = found ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ the two passes
// r = s R x + t - y
__device__ __forceinline__ double sim3_residual2(const Sim3Model& m, const double (&x)[3], const double (&y)[3]) {
  const double e0 = (dot3(m.R, x) * m.s + m.t[0]) - y[0];
  const double e1 = (dot3(m.R + 3, x) * m.s + m.t[1]) - y[1];
  const double e2 = (dot3(m.R + 6, x) * m.s + m.t[2]) - y[2];
  return (e0 * e0 + e1 * e1) + e2 * e2;
}

struct Sim3Sums {
  double cost;      // truncated cost of the model (+inf without one)
  int nact, nfin;   // active rows, finite rows
  double c[6];      // sums of x and y over the active rows
};

// the truncated cost of m and the count and sums of its active rows (has: a model; without one every finite row is active).
// rowf(i, x, y) -> whether row i is finite, and its points.  LM_THREADS threads, every thread returns the same bits.
template <class RowF>
__device__ __forceinline__ Sim3Sums sim3_pass_cost(const Sim3Model& m, bool has, int n, double thr2, RowF rowf, double* sh, int* shc) {
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // r^2, x, y, finite rows
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    double x[3], y[3];
    if (!rowf(i, x, y)) continue;
    v[7] = v[7] + 1.0;
    const double r2 = has ? sim3_residual2(m, x, y) : 0.0;
    if (r2 < thr2) {
      v[0] = v[0] + r2;
#pragma unroll
      for (int a = 0; a < 3; ++a) { v[1 + a] = v[1 + a] + x[a]; v[4 + a] = v[4 + a] + y[a]; }
      ++cnt;
    }
  }
  lm_reduce(v, cnt, sh, shc);
  Sim3Sums o;
  o.nact = cnt;
  o.nfin = (int)v[7];
  o.cost = has ? (isfinite(thr2) ? v[0] + thr2 * (double)(o.nfin - cnt) : v[0]) : INFINITY;
#pragma unroll
  for (int a = 0; a < 6; ++a) o.c[a] = v[1 + a];
  return o;
}

// the closed form on the active rows of m: centred moments about their centroids (S.c / S.nact), then sim3_from_moments
template <class RowF>
__device__ __forceinline__ bool sim3_pass_fit(const Sim3Model& m, bool has, const Sim3Sums& S, int n, double thr2, bool with_scale,
                                              RowF rowf, double* sh, int* shc, Sim3Model& out) {
  double xb[3], yb[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { xb[a] = S.c[a] / (double)S.nact; yb[a] = S.c[3 + a] / (double)S.nact; }
  double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // sxx, C
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    double x[3], y[3];
    if (!rowf(i, x, y)) continue;
    const double r2 = has ? sim3_residual2(m, x, y) : 0.0;
    if (r2 < thr2) {
      double dx[3], dy[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) { dx[a] = x[a] - xb[a]; dy[a] = y[a] - yb[a]; }
      v[0] = v[0] + dot3(dx, dx);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[1 + 3 * a + c] = v[1 + 3 * a + c] + dy[a] * dx[c];
      ++cnt;
    }
  }
  lm_reduce(v, cnt, sh, shc);
  double C[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) C[e] = v[1 + e];
  return sim3_from_moments((double)cnt, xb, yb, v[0], C, with_scale, out);
}

struct Sim3Fit {
  int steps, evals, nact;
  double cost0, cost;
};

// the whole loop from the start m (has: there is one), which becomes the final model.  Every branch is uniform over the workgroup.
template <class RowF>
__device__ __forceinline__ Sim3Fit sim3_fit(Sim3Model& m, bool& has, int n, double thr2, int max_steps, bool with_scale, RowF rowf,
                                            double* sh, int* shc) {
  Sim3Sums cur = sim3_pass_cost(m, has, n, thr2, rowf, sh, shc);
  Sim3Fit f = {0, 1, has ? cur.nact : 0, cur.cost, cur.cost};
  while (f.steps < max_steps && cur.nact >= SIM3_MIN_ROWS) {
    Sim3Model cand;
    if (!sim3_pass_fit(m, has, cur, n, thr2, with_scale, rowf, sh, shc, cand)) break;
    const Sim3Sums next = sim3_pass_cost(cand, true, n, thr2, rowf, sh, shc);
    ++f.evals;
    if (!(next.cost < cur.cost)) break;
    m = cand;
    has = true;
    cur = next;
    ++f.steps;
    f.nact = cur.nact;
    f.cost = cur.cost;
  }
  return f;
}

// ------------------------------------------------------------------------------------------------------------ refinement
__global__ __launch_bounds__(LM_THREADS) void sim3_refine_kernel(const double* __restrict__ s_in, const double* __restrict__ R_in,
                                                                 const double* __restrict__ t_in, const float* __restrict__ src,
                                                                 const float* __restrict__ dst, const int* __restrict__ counts,
                                                                 const unsigned char* __restrict__ valid, int N, double thr,
                                                                 int max_steps, int with_scale, double* __restrict__ out_s,
                                                                 double* __restrict__ out_R, double* __restrict__ out_t,
                                                                 unsigned char* __restrict__ mask, int* __restrict__ out_info,
                                                                 double* __restrict__ out_cost) {
  __shared__ double sh[LM_WAVES * 10];
  __shared__ int shc[LM_WAVES];
  const int b = blockIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  const float* xs = src + (long)b * N * 3;
  const float* ys = dst + (long)b * N * 3;
  // the normalisation of Sim3::normalise (the waves' sums in lm_reduce's order)
  SimNorm nrm = SimNorm::identity(with_scale);
  double sum[6] = {0, 0, 0, 0, 0, 0};
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    double x[3], y[3];
    nrm.apply(xs + 3 * (long)i, ys + 3 * (long)i, x, y);
    if (SimNorm::finite(x, y)) {
#pragma unroll
      for (int a = 0; a < 3; ++a) { sum[a] += x[a]; sum[3 + a] += y[a]; }
      ++cnt;
    }
  }
  lm_reduce(sum, cnt, sh, shc);
  double c[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) c[a] = sum[a] / cnt;
  double ds[2] = {0.0, 0.0};
  int cnt2 = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    double x[3], y[3];
    nrm.apply(xs + 3 * (long)i, ys + 3 * (long)i, x, y);
    if (SimNorm::finite(x, y)) {
      const double a0 = x[0] - c[0], a1 = x[1] - c[1], a2 = x[2] - c[2];
      const double b0 = y[0] - c[3], b1 = y[1] - c[4], b2 = y[2] - c[5];
      ds[0] += sqrt((a0 * a0 + a1 * a1) + a2 * a2);
      ds[1] += sqrt((b0 * b0 + b1 * b1) + b2 * b2);
      ++cnt2;
    }
  }
  lm_reduce(ds, cnt2, sh, shc);
  nrm.set(c, ds[0] / cnt, ds[1] / cnt);

  const bool start = s_in != nullptr;
  bool ok = (!valid || valid[b]) && cnt >= SIM3_MIN_ROWS && isfinite(nrm.sx) && isfinite(nrm.sy);
  Sim3Model m;
  double sin_ = 0.0, Rin[9], tin[3];
#pragma unroll
  for (int e = 0; e < 9; ++e) Rin[e] = start ? R_in[(long)b * 9 + e] : 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) tin[r] = start ? t_in[(long)b * 3 + r] : 0.0;
  if (start) {
    sin_ = s_in[b];
    ok = ok && isfinite(sin_);
#pragma unroll
    for (int e = 0; e < 9; ++e) ok = ok && isfinite(Rin[e]);
#pragma unroll
    for (int r = 0; r < 3; ++r) ok = ok && isfinite(tin[r]);
  }
  // s' = s sy / sx, t' = sy (s R cx + t - cy)
  m.s = sin_ * (nrm.sy / nrm.sx);
#pragma unroll
  for (int e = 0; e < 9; ++e) m.R[e] = Rin[e];
#pragma unroll
  for (int r = 0; r < 3; ++r) m.t[r] = nrm.sy * ((sin_ * dot3(Rin + 3 * r, nrm.cx) + tin[r]) - nrm.cy[r]);
  const double thr_n = thr * nrm.sy, thr2 = thr_n * thr_n;
  auto rowf = [&](int i, double (&x)[3], double (&y)[3]) {
    nrm.apply(xs + 3 * (long)i, ys + 3 * (long)i, x, y);
    return SimNorm::finite(x, y);
  };
  bool has = start;
  Sim3Fit fit = {0, 0, 0, NAN, NAN};
  // uniform over the workgroup, like every branch of the loop: all threads hold the same values
  if (ok) fit = sim3_fit(m, has, n, thr2, max_steps, with_scale != 0, rowf, sh, shc);
  if (threadIdx.x == 0) {
    // without an accepted step the input comes back untouched (zeros where there was none)
    double s, t[3];
    nrm.denormalise(m.s, m.R, m.t, s, t);
    out_s[b] = fit.steps ? s : sin_;
    for (int e = 0; e < 9; ++e) out_R[(long)b * 9 + e] = fit.steps ? m.R[e] : Rin[e];
    for (int r = 0; r < 3; ++r) out_t[(long)b * 3 + r] = fit.steps ? t[r] : tin[r];
    out_info[b * 4] = fit.steps;
    out_info[b * 4 + 1] = fit.evals;
    out_info[b * 4 + 2] = fit.nact;
    out_info[b * 4 + 3] = ok ? 1 : 0;
    // in the destination's squared units
    out_cost[b * 2] = fit.cost0 / (nrm.sy * nrm.sy);
    out_cost[b * 2 + 1] = fit.cost / (nrm.sy * nrm.sy);
  }
  // the rows active under the model returned
  for (int i = threadIdx.x; i < N; i += LM_THREADS) {
    bool in = false;
    if (ok && has && i < n) {
      double x[3], y[3];
      in = rowf(i, x, y) && sim3_residual2(m, x, y) < thr2;
    }
    mask[(long)b * N + i] = in ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------------------ trajectory error
// the camera centre -R^T t
__device__ __forceinline__ void camera_centre(const double* R, const double* t, double (&c)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) c[j] = -((R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2]);
}

__global__ __launch_bounds__(LM_THREADS) void sim3_trajectory_kernel(const double* __restrict__ R, const double* __restrict__ t,
                                                                     const double* __restrict__ Rg, const double* __restrict__ tg,
                                                                     const unsigned char* __restrict__ view_ok, int V, int with_scale,
                                                                     double* __restrict__ out_s, double* __restrict__ out_R,
                                                                     double* __restrict__ out_t, double* __restrict__ out_ce,
                                                                     double* __restrict__ out_re, double* __restrict__ out_rmse) {
  __shared__ double sh[LM_WAVES * 10];
  __shared__ int shc[LM_WAVES];
  const int b = blockIdx.x;
  const long o = (long)b * V;
  auto centres = [&](int i, double (&x)[3], double (&y)[3]) {
    camera_centre(R + (o + i) * 9, t + (o + i) * 3, x);
    camera_centre(Rg + (o + i) * 9, tg + (o + i) * 3, y);
    return SimNorm::finite(x, y);
  };
  auto rowf = [&](int i, double (&x)[3], double (&y)[3]) { return centres(i, x, y) && (!view_ok || view_ok[o + i]); };
  Sim3Model m;
  m.s = 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) m.R[e] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) m.t[r] = 0.0;
  bool has = false;
  const Sim3Fit fit = sim3_fit(m, has, V, INFINITY, 1, with_scale != 0, rowf, sh, shc);
  const bool ok = fit.steps == 1;
  double e2[1] = {0.0};
  int cnt = 0;
  for (int i = threadIdx.x; i < V; i += LM_THREADS) {
    double x[3], y[3];
    const bool fin = centres(i, x, y);
    const double r2 = sim3_residual2(m, x, y);
    if (rowf(i, x, y)) {
      e2[0] = e2[0] + r2;
      ++cnt;
    }
    // M = R_c R^T R_gt^T; sin of its angle from its antisymmetric part, cos from its trace
    const double* Rc = R + (o + i) * 9;
    const double* Rt = Rg + (o + i) * 9;
    double Rn[9], M[9];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) Rn[3 * p + q] = dot3(Rc + 3 * p, m.R + 3 * q);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) M[3 * p + q] = dot3(Rn + 3 * p, Rt + 3 * q);
    const double a0 = M[7] - M[5], a1 = M[2] - M[6], a2 = M[3] - M[1];
    const double sn = 0.5 * sqrt((a0 * a0 + a1 * a1) + a2 * a2), cs = 0.5 * (((M[0] + M[4]) + M[8]) - 1.0);
    out_ce[o + i] = ok && fin ? sqrt(r2) : NAN;
    out_re[o + i] = ok ? atan2(sn, cs) * (180.0 / M_PI) : NAN;
  }
  lm_reduce(e2, cnt, sh, shc);
  if (threadIdx.x == 0) {
    out_s[b] = ok ? m.s : NAN;
    for (int e = 0; e < 9; ++e) out_R[(long)b * 9 + e] = ok ? m.R[e] : NAN;
    for (int r = 0; r < 3; ++r) out_t[(long)b * 3 + r] = ok ? m.t[r] : NAN;
    out_rmse[b] = ok ? sqrt(e2[0] / (double)cnt) : NAN;
  }
}

// ------------------------------------------------------------------------------------------------------------ apply
// grid (ceil(N / 256), B): f64 arithmetic, rounded once at the store
__global__ __launch_bounds__(256) void sim3_apply_points_kernel(const double* __restrict__ s, const double* __restrict__ R,
                                                                const double* __restrict__ t, const float* __restrict__ pts, int N,
                                                                float* __restrict__ out) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const long row = ((long)b * N + i) * 3;
  const double x[3] = {(double)pts[row], (double)pts[row + 1], (double)pts[row + 2]};
  const double* Rb = R + (long)b * 9;
#pragma unroll
  for (int r = 0; r < 3; ++r) out[row + r] = (float)(dot3(Rb + 3 * r, x) * s[b] + t[(long)b * 3 + r]);
}

// grid (ceil(V / 64), B): R_c' = R_c R^T, t_c' = s t_c - R_c' t
__global__ __launch_bounds__(64) void sim3_apply_cameras_kernel(const double* __restrict__ s, const double* __restrict__ R,
                                                                const double* __restrict__ t, const double* __restrict__ cam_R,
                                                                const double* __restrict__ cam_t, int V, double* __restrict__ out_R,
                                                                double* __restrict__ out_t) {
  const int b = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
  if (i >= V) return;
  const long v = (long)b * V + i;
  const double* Rb = R + (long)b * 9;
  const double* tb = t + (long)b * 3;
  double Rn[9];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      Rn[3 * p + q] = dot3(cam_R + v * 9 + 3 * p, Rb + 3 * q);
      out_R[v * 9 + 3 * p + q] = Rn[3 * p + q];
    }
#pragma unroll
  for (int p = 0; p < 3; ++p) out_t[v * 3 + p] = s[b] * cam_t[v * 3 + p] - dot3(Rn + 3 * p, tb);
}

// ------------------------------------------------------------------------------------------------------------ depth rows
// pixel (u, v) through depth d, camera K and pose (R, t), x_cam = R X + t, into the pose's world: R^T (x_cam - t)
__device__ __forceinline__ void back_project(double px, double py, double d, const double* K, const double* R, const double* t,
                                             double (&X)[3]) {
  const double c0 = (px - K[2]) / K[0] * d - t[0], c1 = (py - K[5]) / K[4] * d - t[1], c2 = d - t[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) X[j] = (R[j] * c0 + R[3 + j] * c1) + R[6 + j] * c2;
}

// grid (ceil(N / 256), B), N = nh nw rows in row-major order
__global__ __launch_bounds__(256) void depth_rows_kernel(const float* __restrict__ da, const float* __restrict__ db,
                                                         const double* __restrict__ K, const double* __restrict__ Ra,
                                                         const double* __restrict__ ta, const double* __restrict__ Rb,
                                                         const double* __restrict__ tb, int H, int W, int step, int nh, int nw,
                                                         float* __restrict__ src, float* __restrict__ dst) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nh * nw) return;
  const int v = (i / nw) * step, u = (i % nw) * step;  // v <= (nh - 1) step < H, u < W
  const long pix = ((long)b * H + v) * W + u;
  const double za = da[pix], zb = db[pix];
  const bool ok = isfinite(za) && isfinite(zb) && za > 0 && zb > 0;
  const double px = (double)u + 0.5, py = (double)v + 0.5;
  double Xa[3], Xb[3];
  back_project(px, py, za, K + (long)b * 9, Ra + (long)b * 9, ta + (long)b * 3, Xa);
  back_project(px, py, zb, K + (long)b * 9, Rb + (long)b * 9, tb + (long)b * 3, Xb);
  const long row = ((long)b * nh * nw + i) * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    src[row + j] = ok ? (float)Xb[j] : NAN;
    dst[row + j] = ok ? (float)Xa[j] : NAN;
  }
}

}  // namespace

extern "C" long roma_op_align_points_workspace(int B, int N) { return workspace_bytes<Sim3, CountScoring>(B, N); }

extern "C" int roma_op_align_points(const float* src, const float* dst, const int* counts, const unsigned long long* seeds, int B, int N,
                                    float thr, double conf, int max_iters, int with_scale, double* out_scale, double* out_r,
                                    double* out_t, unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* ws,
                                    long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  if (check_args<CountScoring>("align_points", "conf", src && dst && seeds && out_scale && out_r && out_t && out_mask && out_ok && out_info && ws,
                               B, N, thr, conf, max_iters, 0, ws_bytes, (size_t)roma_op_align_points_workspace(B, N)))
    return -1;
  ROMA_REQUIRE(with_scale == 0 || with_scale == 1, "align_points: with_scale must be 0 or 1");
  return ransac_run<Sim3, CountScoring>({src, dst, with_scale}, counts, seeds, nullptr, B, N, thr, conf, max_iters, 0,
                                        {out_scale, out_r, out_t}, out_mask, out_ok, out_info, nullptr, ws, s);
}

extern "C" int roma_op_similarity_minimal(const double* X, const double* Y, int S, int with_scale, double* out_scale, double* out_r,
                                          double* out_t, int* out_n, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(X && Y && out_scale && out_r && out_t && out_n, "similarity_minimal: null pointer");
  ROMA_REQUIRE(S > 0 && S <= (1 << 24), "similarity_minimal: need 0 < S <= 2^24");
  ROMA_REQUIRE(with_scale == 0 || with_scale == 1, "similarity_minimal: with_scale must be 0 or 1");
  hipLaunchKernelGGL(sim3_minimal_kernel, dim3((S + 63) / 64), dim3(64), 0, s, X, Y, S, with_scale, out_scale, out_r, out_t, out_n);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_refine_similarity(const double* scale_in, const double* R_in, const double* t_in, const float* src, const float* dst,
                                         const int* counts, const unsigned char* valid, int B, int N, double thr, int max_steps,
                                         int with_scale, double* out_scale, double* out_r, double* out_t, unsigned char* out_mask,
                                         int* out_info, double* out_cost, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(src && dst && out_scale && out_r && out_t && out_mask && out_info && out_cost, "refine_similarity: null pointer");
  ROMA_REQUIRE((scale_in && R_in && t_in) || (!scale_in && !R_in && !t_in),
               "refine_similarity: scale, R and t go together (all NULL: no start)");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16),
               "refine_similarity: need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(thr > 0, "refine_similarity: threshold must be positive (+inf: no truncation)");
  ROMA_REQUIRE(max_steps >= 0 && max_steps <= (1 << 16), "refine_similarity: need 0 <= max_steps <= 65536");
  ROMA_REQUIRE(with_scale == 0 || with_scale == 1, "refine_similarity: with_scale must be 0 or 1");
  hipLaunchKernelGGL(sim3_refine_kernel, dim3(B), dim3(LM_THREADS), 0, s, scale_in, R_in, t_in, src, dst, counts, valid, N, thr, max_steps,
                     with_scale, out_scale, out_r, out_t, out_mask, out_info, out_cost);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_apply_similarity(const double* scale, const double* R_, const double* t, const float* points, int N,
                                        const double* cam_R, const double* cam_t, int V, int B, float* out_points, double* out_cam_R,
                                        double* out_cam_t, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(scale && R_ && t, "apply_similarity: null pointer");
  ROMA_REQUIRE(B > 0 && B <= 65535 && N >= 0 && V >= 0 && (long)B * N < (1l << 31) && (long)B * V < (1l << 31),
               "apply_similarity: need 0 < B <= 65535, 0 <= N, 0 <= V, B * N < 2^31, B * V < 2^31");
  ROMA_REQUIRE(N == 0 ? !points && !out_points : points && out_points, "apply_similarity: points and out_points go with N > 0");
  ROMA_REQUIRE(V == 0 ? !cam_R && !cam_t && !out_cam_R && !out_cam_t : cam_R && cam_t && out_cam_R && out_cam_t,
               "apply_similarity: the four camera arrays go with V > 0");
  if (N > 0) {
    hipLaunchKernelGGL(sim3_apply_points_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, scale, R_, t, points, N, out_points);
    ROMA_LAUNCH_CHECK();
  }
  if (V > 0) {
    hipLaunchKernelGGL(sim3_apply_cameras_kernel, dim3((V + 63) / 64, B), dim3(64), 0, s, scale, R_, t, cam_R, cam_t, V, out_cam_R,
                       out_cam_t);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int roma_op_depth_rows(const float* depth_a, const float* depth_b, const double* K, const double* Ra, const double* ta,
                                  const double* Rb, const double* tb, int B, int H, int W, int step, float* out_src, float* out_dst,
                                  void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(depth_a && depth_b && K && Ra && ta && Rb && tb && out_src && out_dst, "depth_rows: null pointer");
  ROMA_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long)B * H * W < (1l << 31),
               "depth_rows: need 0 < B <= 65535, positive image sizes, B * H * W < 2^31");
  ROMA_REQUIRE(step >= 1, "depth_rows: step must be at least 1");
  const int nh = (H + step - 1) / step, nw = (W + step - 1) / step;
  hipLaunchKernelGGL(depth_rows_kernel, dim3((nh * nw + 255) / 256, B), dim3(256), 0, s, depth_a, depth_b, K, Ra, ta, Rb, tb, H, W, step,
                     nh, nw, out_src, out_dst);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_trajectory_error(const double* R_, const double* t, const double* R_gt, const double* t_gt,
                                        const unsigned char* view_ok, int B, int V, int with_scale, double* out_scale, double* out_r,
                                        double* out_t, double* out_centre_err, double* out_rot_err_deg, double* out_rmse, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(R_ && t && R_gt && t_gt && out_scale && out_r && out_t && out_centre_err && out_rot_err_deg && out_rmse,
               "trajectory_error: null pointer");
  ROMA_REQUIRE(B > 0 && V > 0 && (long)B * V < (1l << 31) && B <= (1 << 16), "trajectory_error: need 0 < B <= 65536, 0 < V, B * V < 2^31");
  ROMA_REQUIRE(with_scale == 0 || with_scale == 1, "trajectory_error: with_scale must be 0 or 1");
  hipLaunchKernelGGL(sim3_trajectory_kernel, dim3(B), dim3(LM_THREADS), 0, s, R_, t, R_gt, t_gt, view_ok, V, with_scale, out_scale, out_r,
                     out_t, out_centre_err, out_rot_err_deg, out_rmse);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
