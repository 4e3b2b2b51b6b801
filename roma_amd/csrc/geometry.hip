// Homography (H) and fundamental-matrix (F) models of the device RANSAC (ransac.h) - what the reference's demos hand to OpenCV
// after `sample()`: cv2.findHomography(..., RANSAC) (HPatches benchmark) and cv2.findFundamentalMat(..., FM_RANSAC)
// (demo_fundamental).  tools/geometry_ref.py restates this file in numpy float64 step by step.
//
// What H and F add to the shared pipeline (Hartley<M>):
//   normalise   Hartley normalisation of each image (centroid to 0, mean distance to sqrt 2) over the finite rows, f64
//               fixed-order reductions; thresholds thr * s per image.
//   hypothesis  one thread per hypothesis: its sample's rows normalised in f64 (ransac.h: load_sample), then the 4-point DLT as
//               an 8 x 8 solve with OpenCV's checkSubset (1 slot), or 7-point null space + cubic (up to 3 slots), f64.
//   res_terms   the f32 scoring's terms linear in the model: reprojection error in image B and p_z (H), the epipolar terms (F).
//   inlier      (CountScoring) from them: reprojection error in image B (H); distances to both epipolar lines, each image with
//               its own scale (F).
//   residual2   (MagsacScoring) from them: squared pixel residuals - reprojection error in image B (H), Sampson distance (F).
//   refit       (CountScoring) up to REFINE_ITERS times: 9 x 9 normal equations in f64 on the current inliers (ransac.h:
//               normal_equations), smallest eigenvector by one-sided Jacobi on one wave (jacobi_min_vec); rank 2 for F.
//   wrefit      (MagsacScoring) the same with the rows weighted by the MAGSAC++ weights of the current model (one IRLS step).
//   model_out   de-normalised in f64 (H = Tb^-1 H_n Ta, F = Tb^T F_n Ta), scaled so that [2, 2] = 1.  Info rows of RANSAC_INFO
//               and MAGSAC_INFO ints.
#include "../../include/roma_hip.h"
#include "geometry.h"
#include "ransac.h"

namespace roma {
namespace {

constexpr int RANSAC_INFO = 6;                // ints per pair in roma_op_ransac's out_info
constexpr int MAGSAC_INFO = RANSAC_INFO + 1;  // in roma_op_magsac's: the RANSAC_INFO entries and the LO steps accepted
constexpr int MAGSAC_MAX_LO = 64;             // largest lo_iters

constexpr double COLLINEAR_EPS = 1e-4;  // |sin| of a triple's angle below which the triple counts as collinear
constexpr double CUBIC_EPS = 1e-12;     // relative size below which a leading coefficient of the cubic is zero

// ------------------------------------------------------------------------------------------------------------ f64 helpers
__device__ __forceinline__ void unit_norm(double* m) {
  double s = 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) s += m[k] * m[k];
  const double inv = 1.0 / sqrt(s);
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] *= inv;
}

__device__ __forceinline__ bool all_finite(const double* m) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) ok &= isfinite(m[k]);
  return ok;
}

// real roots of c3 x^3 + c2 x^2 + c1 x + c0, ascending; their number (0 .. 3).  Closed form (trigonometric / Cardano), then
// two Newton steps on the cubic.
__device__ int solve_cubic(double c3, double c2, double c1, double c0, double* x) {
  const double cmax = fmax(fmax(fabs(c3), fabs(c2)), fmax(fabs(c1), fabs(c0)));
  if (!(cmax > 0) || !isfinite(cmax)) return 0;
  int n;
  if (fabs(c3) <= CUBIC_EPS * cmax) {
    if (fabs(c2) <= CUBIC_EPS * cmax) {
      if (fabs(c1) <= CUBIC_EPS * cmax) return 0;
      x[0] = -c0 / c1;
      n = 1;
    } else {
      const double d = c1 * c1 - 4 * c2 * c0;
      if (d < 0) return 0;
      const double q = -0.5 * (c1 + copysign(sqrt(d), c1));
      const double r0 = q / c2, r1 = q != 0 ? c0 / q : r0;
      x[0] = fmin(r0, r1);
      x[1] = fmax(r0, r1);
      n = 2;
    }
  } else {
    const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
    const double Q = (a * a - 3 * b) / 9, Rr = (2 * a * a * a - 9 * a * b + 27 * c) / 54;
    const double Q3 = Q * Q * Q;
    if (Rr * Rr < Q3) {
      const double th = acos(Rr / sqrt(Q3)), sq = -2 * sqrt(Q), a3 = a / 3;
      x[0] = sq * cos(th / 3) - a3;
      x[1] = sq * cos((th + 2 * M_PI) / 3) - a3;
      x[2] = sq * cos((th - 2 * M_PI) / 3) - a3;
      n = 3;
    } else {
      const double A = -copysign(cbrt(fabs(Rr) + sqrt(Rr * Rr - Q3)), Rr);
      const double Bq = A != 0 ? Q / A : 0;
      x[0] = (A + Bq) - a / 3;
      n = 1;
    }
  }
  for (int k = 0; k < n; ++k) {
    double r = x[k];
    for (int it = 0; it < 2; ++it) {
      const double p = ((c3 * r + c2) * r + c1) * r + c0, dp = (3 * c3 * r + 2 * c2) * r + c1;
      if (dp != 0) {
        const double r1 = r - p / dp;
        if (isfinite(r1)) r = r1;
      }
    }
    x[k] = r;
  }
  if (n == 3) {  // sort
    double t;
    if (x[0] > x[1]) { t = x[0]; x[0] = x[1]; x[1] = t; }
    if (x[1] > x[2]) { t = x[1]; x[1] = x[2]; x[2] = t; }
    if (x[0] > x[1]) { t = x[0]; x[0] = x[1]; x[1] = t; }
  } else if (n == 2 && x[0] > x[1]) {
    const double t = x[0]; x[0] = x[1]; x[1] = t;
  }
  return n;
}

// ------------------------------------------------------------------------------------------------------------ minimal solvers
// OpenCV's checkSubset for the homography: no triple of the sample (nearly) collinear in either image, and the four triples
// keep (all of them) or flip (all of them) their orientation between the images.
__device__ __forceinline__ bool h_subset_ok(const double* xa, const double* ya, const double* xb, const double* yb) {
  constexpr int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
  int neg = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tt[t][0], j = tt[t][1], k = tt[t][2];
    const double ax1 = xa[j] - xa[i], ay1 = ya[j] - ya[i], ax2 = xa[k] - xa[i], ay2 = ya[k] - ya[i];
    const double bx1 = xb[j] - xb[i], by1 = yb[j] - yb[i], bx2 = xb[k] - xb[i], by2 = yb[k] - yb[i];
    const double ca = ax1 * ay2 - ay1 * ax2, cb = bx1 * by2 - by1 * bx2;
    if (!(fabs(ca) > COLLINEAR_EPS * sqrt((ax1 * ax1 + ay1 * ay1) * (ax2 * ax2 + ay2 * ay2)))) return false;
    if (!(fabs(cb) > COLLINEAR_EPS * sqrt((bx1 * bx1 + by1 * by1) * (bx2 * bx2 + by2 * by2)))) return false;
    neg += ca * cb < 0 ? 1 : 0;
  }
  return neg == 0 || neg == 4;
}

// 4-point DLT with h33 = 1: 8 x 8 solve.  Returns the number of models (0 or 1).
__device__ int solve_h(const double* xa, const double* ya, const double* xb, const double* yb, double (&m)[1][9]) {
  if (!h_subset_ok(xa, ya, xb, yb)) return 0;
  double a[8][9];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = xa[k], y = ya[k], u = xb[k], v = yb[k];
    a[2 * k][0] = x; a[2 * k][1] = y; a[2 * k][2] = 1; a[2 * k][3] = 0; a[2 * k][4] = 0; a[2 * k][5] = 0;
    a[2 * k][6] = -u * x; a[2 * k][7] = -u * y; a[2 * k][8] = u;
    a[2 * k + 1][0] = 0; a[2 * k + 1][1] = 0; a[2 * k + 1][2] = 0; a[2 * k + 1][3] = x; a[2 * k + 1][4] = y; a[2 * k + 1][5] = 1;
    a[2 * k + 1][6] = -v * x; a[2 * k + 1][7] = -v * y; a[2 * k + 1][8] = v;
  }
  if (!gauss_jordan(a)) return 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) m[0][k] = a[k][8];
  m[0][8] = 1;
  return all_finite(m[0]) ? 1 : 0;
}

// 7-point: two-dimensional null space of the 7 x 9 system x_B^T F x_A = 0, then det(alpha F1 + (1 - alpha) F2) = 0.
// Returns the number of models (0 .. 3), each with unit Frobenius norm, in ascending order of alpha.
__device__ int solve_f(const double* xa, const double* ya, const double* xb, const double* yb, double (&m)[3][9]) {
  double a[7][9];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double x = xa[k], y = ya[k], u = xb[k], v = yb[k];
    a[k][0] = u * x; a[k][1] = u * y; a[k][2] = u; a[k][3] = v * x; a[k][4] = v * y; a[k][5] = v;
    a[k][6] = x; a[k][7] = y; a[k][8] = 1;
  }
  if (!gauss_jordan(a)) return 0;
  double f1[9], f2[9], d[9], g[9];
#pragma unroll
  for (int k = 0; k < 7; ++k) { f1[k] = -a[k][7]; f2[k] = -a[k][8]; }
  f1[7] = 1; f1[8] = 0; f2[7] = 0; f2[8] = 1;
#pragma unroll
  for (int k = 0; k < 9; ++k) { d[k] = f1[k] - f2[k]; g[k] = f2[k] - d[k]; }
  // det(F2 + alpha D) = c3 alpha^3 + c2 alpha^2 + c1 alpha + c0, from its values at alpha = 0, 1, -1 and det D
  const double c0 = det3(f2), c3 = det3(d), p1 = det3(f1), pm1 = det3(g);
  const double c2 = (p1 + pm1) * 0.5 - c0, c1 = (p1 - pm1) * 0.5 - c3;
  double roots[3];
  const int nr = solve_cubic(c3, c2, c1, c0, roots);
  int n = 0;
  for (int r = 0; r < nr; ++r) {
    const double al = roots[r], mu = 1 - al;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = al * f1[k] + mu * f2[k];
    unit_norm(f);
    if (!all_finite(f)) continue;
#pragma unroll
    for (int k = 0; k < 9; ++k) m[n][k] = f[k];
    ++n;
  }
  return n;
}

// ------------------------------------------------------------------------------------------------------------ model policies
// what H and F share: Hartley normalisation, one thread per hypothesis, the least-squares refit and the de-normalisation.
// Model supplies MODEL, S, SLOTS, REFIT_MIN, NT, res_terms, inlier_from, r2_from and solve.
template <class Model>
struct Hartley : Terms<Model> {
  struct Norm {
    double ca[2], cb[2], sa, sb;  // x_n = (x - c) * s
    __device__ void apply(float2 a, float2 q, double& xa, double& ya, double& xb, double& yb) const {
      xa = (a.x - ca[0]) * sa; ya = (a.y - ca[1]) * sa;
      xb = (q.x - cb[0]) * sb; yb = (q.y - cb[1]) * sb;
    }
  };
  using In = PairIn;
  using Rows = PairRows;
  using Out = double*;  // [B, 9]
  static constexpr int NM = 9, MIN_INLIERS = 1, HYP_THREADS = 64, HYP_LANES = 1, REFINE_ITERS = 3, INFO = RANSAC_INFO;
  static constexpr int MAG_INFO = MAGSAC_INFO;
  // score all (at most 3) slots of a hypothesis, used or not: every model's coefficients then stay in registers across the
  // point loop, where a branch per slot reloads them (35 % slower for F); unused slots hold zeros and their counts are dropped
  static constexpr bool SCORE_EVERY_SLOT = true;

  __device__ static double mag_thr2(const Norm&, float thr) { return (double)thr * thr; }  // residuals in pixels

  __device__ static void res_scales(const Norm& nm, float& sa2, float& sb2) {  // the scales of M::residual2
    sa2 = (float)(nm.sa * nm.sa);
    sb2 = (float)(nm.sb * nm.sb);
  }

  // every thread of the workgroup: the pair's normalisation over its finite rows; pts written only for a valid pair
  __device__ static bool normalise(PairIn in, int n, const double*, float thr, double* sh, PairRows rows, Norm& nm, float& t2a,
                                   float& t2b) {
    const float2 *A = in.a, *Bp = in.b;
    float4* pts = rows.p;
    const HartleyMoments m = hartley_moments(n, [&](int i, double& ax, double& ay, double& bx, double& by) {
      const float2 a = A[i], q = Bp[i];
      ax = a.x; ay = a.y; bx = q.x; by = q.y;
      return finite_row(a.x, a.y, q.x, q.y);
    }, sh);
    const bool valid = m.ok(Model::S);
    if (valid) {
      for (int i = threadIdx.x; i < n; i += 256) {
        const float2 a = A[i], q = Bp[i];
        float4 o = make_float4(NAN, NAN, NAN, NAN);
        if (finite_row(a.x, a.y, q.x, q.y))
          o = make_float4((float)((a.x - m.cax) * m.sa), (float)((a.y - m.cay) * m.sa), (float)((q.x - m.cbx) * m.sb),
                          (float)((q.y - m.cby) * m.sb));
        pts[i] = o;
      }
    }
    nm.ca[0] = m.cax; nm.ca[1] = m.cay; nm.cb[0] = m.cbx; nm.cb[1] = m.cby; nm.sa = m.sa; nm.sb = m.sb;
    const double ta = (double)thr * m.sa, tb = (double)thr * m.sb;
    t2a = (float)(ta * ta);
    t2b = (float)(tb * tb);
    return valid;
  }

  template <int S>  // Model::S (Model is not complete here)
  __device__ static void hypothesis(PairIn in, const int (&idx)[S], bool act, const Norm& nrm, int g, int, const Slots& sl) {
    double xa[S], ya[S], xb[S], yb[S];
    act = load_sample(in, idx, act, nrm, xa, ya, xb, yb);
    double m[Model::SLOTS][9];
    const int nm = act ? Model::solve(xa, ya, xb, yb, m) : 0;
    sl.n[g] = nm;
#pragma unroll
    for (int r = 0; r < Model::SLOTS; ++r) {
      if (r >= nm) {
#pragma unroll
        for (int k = 0; k < 9; ++k) m[r][k] = 0;
      }
      store_model(m[r], (long)g * Model::SLOTS + r, sl);
    }
  }

  // least-squares refit (normalised DLT / normalised 8-point + rank 2); A, Bp: the pair's rows.  W = false: the rows of the
  // current mask, with at least REFIT_MIN inliers (RANSAC refinement).  W = true: the MAGSAC++ IRLS step - the normal equations
  // weighted by w(V) of the current model over the rows of positive weight, at least REFIT_MIN of them; pts: the pair's
  // normalised f32 rows the scoring reads.
  template <bool W>
  __device__ static void fit(const float2* A, const float2* Bp, PairState<Model>& P, const unsigned char* mask, const float4* pts,
                             const MagState* S) {
    constexpr bool H = Model::MODEL == RANSAC_HOMOGRAPHY;
    __shared__ double M[9][9];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (P.stop) return;
    if (W ? P.best_h < 0 : P.best < Model::REFIT_MIN) {
      if (t == 0) { P.stop = 1; P.cand_ok = 0; }
      return;
    }
    const double cax = P.nrm.ca[0], cay = P.nrm.ca[1], cbx = P.nrm.cb[0], cby = P.nrm.cb[1], sa = P.nrm.sa, sb = P.nrm.sb;
    const int rows = normal_equations<W, H>(P.n, [&](int i, double& wt) {
      if constexpr (W) {
        float w;
        magsac_rho(Model::residual2(P.curf, pts[i], S->sa2, S->sb2) * S->vs, w);
        wt = w;
        return w > 0.f;
      } else {
        return mask[i] != 0;
      }
    }, [&](int i, double (&r1)[9], double (&r2)[9]) {
      const float2 a = A[i], q = Bp[i];
      const double x = (a.x - cax) * sa, y = (a.y - cay) * sa, u = (q.x - cbx) * sb, v = (q.y - cby) * sb;
      if constexpr (H) {
        const double h1[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, -u}, h2[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, -v};
#pragma unroll
        for (int k = 0; k < 9; ++k) { r1[k] = h1[k]; r2[k] = h2[k]; }
      } else {
        const double f1[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1};
#pragma unroll
        for (int k = 0; k < 9; ++k) r1[k] = f1[k];
      }
    }, M);
    if (W && rows < Model::REFIT_MIN) {  // rows of positive weight over the workgroup
      if (t == 0) { P.stop = 1; P.cand_ok = 0; }
      return;
    }
    if (wave != 0) return;
    double col[9], vv[9], h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      col[k] = lane < 9 ? M[k][lane] : 0.0;
      vv[k] = lane == k ? 1.0 : 0.0;
    }
    jacobi_min_vec<9, 10>(col, vv, lane, h);
    if (!H) {  // rank 2: F - (F v)(v^T), v the smallest right singular vector (eigenvector of F^T F)
      double c3[3], v3[3], w3[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int j = lane < 3 ? lane : 0;
        c3[k] = lane < 3 ? h[0 + k] * h[0 + j] + h[3 + k] * h[3 + j] + h[6 + k] * h[6 + j] : 0.0;
        v3[k] = lane == k ? 1.0 : 0.0;
      }
      jacobi_min_vec<3, 4>(c3, v3, lane, w3);
      double f[9];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double fv = h[3 * r] * w3[0] + h[3 * r + 1] * w3[1] + h[3 * r + 2] * w3[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) f[3 * r + k] = h[3 * r + k] - fv * w3[k];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) h[k] = f[k];
    }
    unit_norm(h);
    if (lane == 0) {
      const bool ok = all_finite(h);
      P.cand_ok = ok ? 1 : 0;
      if (ok) {
        for (int k = 0; k < 9; ++k) P.cand[k] = h[k];
        to_f32(P.cand, P.candf);
      } else {
        P.stop = 1;
      }
    }
  }

  __device__ static void refit(const float2* A, const float2* Bp, PairState<Model>& P, const unsigned char* mask) {
    fit<false>(A, Bp, P, mask, nullptr, nullptr);
  }

  __device__ static void wrefit(const float2* A, const float2* Bp, const float4* pts, PairState<Model>& P, const MagState& S) {
    fit<true>(A, Bp, P, nullptr, pts, &S);
  }

  // de-normalise (H = Tb^-1 H_n Ta, F = Tb^T F_n Ta), scale
  __device__ static void model_out(const PairState<Model>& P, bool good, double* out, int b) {
    out += (long)b * 9;
    const Norm& q = P.nrm;
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (good) {
      const double ta[9] = {q.sa, 0, -q.sa * q.ca[0], 0, q.sa, -q.sa * q.ca[1], 0, 0, 1};
      double l[9], tmp[9];
      if (Model::MODEL == RANSAC_HOMOGRAPHY) {
        const double tbi[9] = {1 / q.sb, 0, q.cb[0], 0, 1 / q.sb, q.cb[1], 0, 0, 1};
        for (int k = 0; k < 9; ++k) l[k] = tbi[k];
      } else {
        const double tbt[9] = {q.sb, 0, 0, 0, q.sb, 0, -q.sb * q.cb[0], -q.sb * q.cb[1], 1};
        for (int k = 0; k < 9; ++k) l[k] = tbt[k];
      }
      mat3(l, P.cur, tmp);
      mat3(tmp, ta, m);
      double fro = 0;
      for (int k = 0; k < 9; ++k) fro += m[k] * m[k];
      fro = sqrt(fro);
      const double sc = fabs(m[8]) >= 1e-12 * fro ? m[8] : fro;
      for (int k = 0; k < 9; ++k) m[k] = m[k] / sc;
    }
    for (int k = 0; k < 9; ++k) out[k] = m[k];
  }
};

// The f32 scoring: p = (xa, ya, xb, yb) normalised; terms linear in the model (ransac.h: Terms), the count scoring's test on
// them in multiplication form (no division, NaN never passes) and the MAGSAC++ squared pixel residual; sa2, sb2 the squared
// scales x_n = (x - c) s.
struct Homography : Hartley<Homography> {
  static constexpr int MODEL = RANSAC_HOMOGRAPHY, S = 4, SLOTS = 1, REFIT_MIN = 4, NT = 3;
  // forward reprojection error in image B, |e|^2 / (p_z^2 s_b^2); terms (e_x, e_y, p_z)
  __device__ static void res_terms(const float* m, float4 p, float (&t)[NT]) {
    const float px = fmaf(m[0], p.x, fmaf(m[1], p.y, m[2]));
    const float py = fmaf(m[3], p.x, fmaf(m[4], p.y, m[5]));
    const float pz = fmaf(m[6], p.x, fmaf(m[7], p.y, m[8]));
    t[0] = fmaf(-p.z, pz, px);
    t[1] = fmaf(-p.w, pz, py);
    t[2] = pz;
  }
  __device__ static bool inlier_from(const float (&t)[NT], float, float t2b) {
    return fmaf(t[0], t[0], t[1] * t[1]) < t2b * (t[2] * t[2]);
  }
  __device__ static float r2_from(const float (&t)[NT], float, float sb2) {
    return fmaf(t[0], t[0], t[1] * t[1]) / (t[2] * t[2] * sb2);
  }
  __device__ static int solve(const double* xa, const double* ya, const double* xb, const double* yb, double (&m)[SLOTS][9]) {
    return solve_h(xa, ya, xb, yb, m);
  }
};

struct Fundamental : Hartley<Fundamental> {
  static constexpr int MODEL = RANSAC_FUNDAMENTAL, S = 7, SLOTS = 3, REFIT_MIN = 8, NT = 5;
  // on the epipolar terms (d, l_x, l_y, k_x, k_y).  OpenCV FM_RANSAC: max(d^2 / |F xa|_{1,2}^2, d^2 / |F^T xb|_{1,2}^2) < thr^2,
  // each image with its own scale; Sampson distance d^2 / (s_b^2 |F x_a|_{1,2}^2 + s_a^2 |F^T x_b|_{1,2}^2), exact in pixels
  // (x_b^T F x_a = x_nb^T F_n x_na)
  __device__ static void res_terms(const float* m, float4 p, float (&t)[NT]) { epipolar_terms(m, p, t); }
  __device__ static bool inlier_from(const float (&t)[NT], float t2a, float t2b) {
    const float d2 = t[0] * t[0];
    return d2 < t2b * fmaf(t[1], t[1], t[2] * t[2]) && d2 < t2a * fmaf(t[3], t[3], t[4] * t[4]);
  }
  __device__ static float r2_from(const float (&t)[NT], float sa2, float sb2) {
    return t[0] * t[0] / fmaf(sb2, fmaf(t[1], t[1], t[2] * t[2]), sa2 * fmaf(t[3], t[3], t[4] * t[4]));
  }
  __device__ static int solve(const double* xa, const double* ya, const double* xb, const double* yb, double (&m)[SLOTS][9]) {
    return solve_f(xa, ya, xb, yb, m);
  }
};

static_assert(MagsacScoring::MAX_STEPS == MAGSAC_MAX_LO);

template <class Sc>
size_t hf_workspace_bytes(int B, int N) {  // one size for both models (the roma_op_*_workspace calls take no model)
  return std::max(workspace_bytes<Homography, Sc>(B, N), workspace_bytes<Fundamental, Sc>(B, N));
}

// the check and dispatch behind roma_op_ransac and roma_op_magsac: `opt` is `refine` or `lo_iters`, out_score NULL without scores
template <class Sc>
int hf_launch(const char* op, int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
              int B, int N, float threshold, double confidence, int max_iters, int opt, double* out_model, unsigned char* out_mask,
              unsigned char* out_ok, int* out_info, double* out_score, void* ws, size_t ws_bytes, hipStream_t s) {
  ROMA_REQUIRE(model == RANSAC_HOMOGRAPHY || model == RANSAC_FUNDAMENTAL,
               std::string(op) + ": model must be 0 (homography) or 1 (fundamental)");
  if (check_args<Sc>(op, "confidence",
                     kpts_a && kpts_b && seeds && out_model && out_mask && out_ok && out_info && (out_score || !Sc::SCORES) && ws, B,
                     N, threshold, confidence, max_iters, opt, ws_bytes, hf_workspace_bytes<Sc>(B, N)))
    return -1;
  const auto run = model == RANSAC_HOMOGRAPHY ? ransac_run<Homography, Sc> : ransac_run<Fundamental, Sc>;
  return run({reinterpret_cast<const float2*>(kpts_a), reinterpret_cast<const float2*>(kpts_b)}, counts, seeds, nullptr, B, N, threshold, confidence, max_iters, opt, out_model, out_mask, out_ok,
             out_info, out_score, ws, s);
}

}  // namespace

extern "C" long roma_op_ransac_workspace(int B, int N) { return (long)hf_workspace_bytes<CountScoring>(B, N); }

extern "C" int roma_op_ransac(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                              int B, int N, float threshold, double confidence, int max_iters, int refine, double* out_model,
                              unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* ws, long ws_bytes, void* stream) {
  return hf_launch<CountScoring>("ransac", model, kpts_a, kpts_b, counts, seeds, B, N, threshold, confidence, max_iters, refine,
                                 out_model, out_mask, out_ok, out_info, nullptr, ws, workspace_size(ws_bytes),
                                 static_cast<hipStream_t>(stream));
}

extern "C" long roma_op_magsac_workspace(int B, int N) { return (long)hf_workspace_bytes<MagsacScoring>(B, N); }

extern "C" int roma_op_magsac(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                              int B, int N, float threshold, double confidence, int max_iters, int lo_iters, double* out_model,
                              unsigned char* out_mask, unsigned char* out_ok, int* out_info, double* out_score, void* ws,
                              long ws_bytes, void* stream) {
  return hf_launch<MagsacScoring>("magsac", model, kpts_a, kpts_b, counts, seeds, B, N, threshold, confidence, max_iters, lo_iters,
                                  out_model, out_mask, out_ok, out_info, out_score, ws, workspace_size(ws_bytes),
                                  static_cast<hipStream_t>(stream));
}

}  // namespace roma
