// Batched RANSAC on the device - what the reference's demos hand to OpenCV after `sample()`: cv2.findHomography(..., RANSAC)
// (HPatches benchmark) and cv2.findFundamentalMat(..., FM_RANSAC) (demo_fundamental).  tools/geometry_ref.py restates this
// file in numpy float64 step by step and is the oracle of the GPU tests.
//
// Per pair b (counts[b] rows of kpts_a / kpts_b; later rows are never read):
//   1. ransac_norm_kernel: Hartley normalisation of each image (centroid to 0, mean distance to sqrt 2) over the finite rows,
//      f64 fixed-order reductions; normalised f32 copies of the points (non-finite rows as NaN); thresholds thr * s per image.
//   2. rounds of RANSAC_ROUND hypotheses, enqueued ceil(max_iters / ROUND) times, no host synchronisation:
//      ransac_hyp_kernel   one thread per hypothesis: sample (counter-based, from (seed_b, h) only), f64 minimal solver
//                          (4-point DLT as an 8 x 8 solve with OpenCV's checkSubset; 7-point null space + cubic, up to 3 roots)
//      ransac_score_kernel one wave per hypothesis: its (up to 3) f32 models against the pair's points, popc(ballot) counts
//      ransac_select_kernel per pair: arg-max (ties: lowest (h, root)), OpenCV's adaptive iteration count, done flag.
//   3. refinement (optional, up to 3 times): ransac_mask_kernel (inliers of the current model), ransac_refit_kernel
//      (9 x 9 normal equations in f64, fixed-order tree reduction, smallest eigenvector by one-sided Jacobi on one wave;
//      rank 2 for F), ransac_accept_kernel (re-score; the refit is kept if its inlier count is not lower).
//   4. ransac_mask_kernel + ransac_finish_kernel: final mask, model de-normalised in f64, ok flag, round / winner info.
// Every flag and counter of the workspace is written with plain stores by one kernel and read by a later launch on the same
// stream: no atomics and no hand-off inside a launch.  Results are bit-identical from run to run and independent of B.
#include "geometry.h"
#include "ransac_common.h"

#include <float.h>
#include <math.h>

// the scoring arithmetic is written with explicit fmaf; nothing else is fused (tools/geometry_ref.py evaluates the same
// expressions in f64)
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int R = RANSAC_ROUND;
constexpr int MAX_ROOTS = 3;          // model slots per hypothesis
constexpr int REFINE_ITERS = 3;
constexpr int JACOBI_SWEEPS = 15;
constexpr double COLLINEAR_EPS = 1e-4;  // |sin| of a triple's angle below which the triple counts as collinear
constexpr double CUBIC_EPS = 1e-12;     // relative size below which a leading coefficient of the cubic is zero
constexpr double JACOBI_TOL = 4 * DBL_EPSILON;

struct PairState {
  double ca[2], cb[2], sa, sb;  // normalisation x_n = (x - c) * s
  double cur[9];                // current model in normalised coordinates
  double cand[9];               // refit candidate
  alignas(16) float curf[12];   // f32 copies the scoring reads
  alignas(16) float candf[12];
  float thr2a, thr2b;           // (thr * s)^2 per image
  int n;                        // rows of the pair: counts[b] clamped to [0, N]
  int valid;                    // enough finite rows for a sample, normalisation well defined
  int best;                     // inlier count of the current model (-1: none yet)
  int best_h, best_root, best_min;  // winning minimal sample and its inlier count
  int needed;                   // adaptive iteration count
  int rounds;                   // rounds executed
  int done;                     // sampling finished for this pair
  int stop;                     // refinement finished for this pair
  int cand_ok;                  // the last refit produced a candidate
};

template <int MODEL> struct Traits;
template <> struct Traits<RANSAC_HOMOGRAPHY> { static constexpr int S = 4, REFIT_MIN = 4; };
template <> struct Traits<RANSAC_FUNDAMENTAL> { static constexpr int S = 7, REFIT_MIN = 8; };

// ------------------------------------------------------------------------------------------------------------ scoring (f32)
// p = (xa, ya, xb, yb) normalised.  Multiplication forms of the reprojection / epipolar tests: no division, NaN never passes.
__device__ __forceinline__ bool inlier_h(const float* m, float4 p, float t2a, float t2b) {
  const float px = fmaf(m[0], p.x, fmaf(m[1], p.y, m[2]));
  const float py = fmaf(m[3], p.x, fmaf(m[4], p.y, m[5]));
  const float pz = fmaf(m[6], p.x, fmaf(m[7], p.y, m[8]));
  const float ex = fmaf(-p.z, pz, px), ey = fmaf(-p.w, pz, py);
  return fmaf(ex, ex, ey * ey) < t2b * (pz * pz);
}

// OpenCV FM_RANSAC: max(d^2 / |F xa|_{1,2}^2, d^2 / |F^T xb|_{1,2}^2) < thr^2, each image with its own scale
__device__ __forceinline__ bool inlier_f(const float* m, float4 p, float t2a, float t2b) {
  const float lx = fmaf(m[0], p.x, fmaf(m[1], p.y, m[2]));
  const float ly = fmaf(m[3], p.x, fmaf(m[4], p.y, m[5]));
  const float lz = fmaf(m[6], p.x, fmaf(m[7], p.y, m[8]));
  const float d = fmaf(p.z, lx, fmaf(p.w, ly, lz));
  const float kx = fmaf(m[0], p.z, fmaf(m[3], p.w, m[6]));
  const float ky = fmaf(m[1], p.z, fmaf(m[4], p.w, m[7]));
  const float d2 = d * d;
  return d2 < t2b * fmaf(lx, lx, ly * ly) && d2 < t2a * fmaf(kx, kx, ky * ky);
}

template <int MODEL>
__device__ __forceinline__ bool inlier(const float* m, float4 p, float t2a, float t2b) {
  return MODEL == RANSAC_HOMOGRAPHY ? inlier_h(m, p, t2a, t2b) : inlier_f(m, p, t2a, t2b);
}

// inlier count of one model over the pair's n points, by one whole wave (wave-uniform result)
template <int MODEL>
__device__ __forceinline__ int wave_count(const float* m, const float4* P, int n, float t2a, float t2b, int lane) {
  int c = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const float4 p = i < n ? P[i] : make_float4(NAN, NAN, NAN, NAN);
    c += __popcll(__ballot(inlier<MODEL>(m, p, t2a, t2b)));
  }
  return c;
}

// ------------------------------------------------------------------------------------------------------------ f64 helpers
__device__ __forceinline__ double det3(const double* f) {
  return f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) + f[2] * (f[3] * f[7] - f[4] * f[6]);
}

__device__ __forceinline__ void to_f32(const double* m, float* mf) {
#pragma unroll
  for (int k = 0; k < 9; ++k) mf[k] = (float)m[k];
#pragma unroll
  for (int k = 9; k < 12; ++k) mf[k] = 0.f;
}

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
__device__ int solve_h(const double* xa, const double* ya, const double* xb, const double* yb, double (&m)[MAX_ROOTS][9]) {
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
__device__ int solve_f(const double* xa, const double* ya, const double* xb, const double* yb, double (&m)[MAX_ROOTS][9]) {
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

// ------------------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void ransac_norm_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb,
                                                          const int* __restrict__ counts, int N, int smin, float thr, int max_iters,
                                                          PairState* __restrict__ st, float4* __restrict__ pts) {
  __shared__ double sh[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  const float2* A = ka + (long)b * N;
  const float2* Bp = kb + (long)b * N;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (int i = t; i < n; i += 256) {
    const float2 a = A[i], q = Bp[i];
    if (finite_row(a.x, a.y, q.x, q.y)) { s0 += a.x; s1 += a.y; s2 += q.x; s3 += q.y; s4 += 1; }
  }
  const double cnt = block_sum(s4, sh);
  const double cax = block_sum(s0, sh) / cnt, cay = block_sum(s1, sh) / cnt;
  const double cbx = block_sum(s2, sh) / cnt, cby = block_sum(s3, sh) / cnt;
  double da = 0, db = 0;
  for (int i = t; i < n; i += 256) {
    const float2 a = A[i], q = Bp[i];
    if (finite_row(a.x, a.y, q.x, q.y)) {
      const double ax = a.x - cax, ay = a.y - cay, bx = q.x - cbx, by = q.y - cby;
      da += sqrt(ax * ax + ay * ay);
      db += sqrt(bx * bx + by * by);
    }
  }
  const double ma = block_sum(da, sh) / cnt, mb = block_sum(db, sh) / cnt;
  const double sa = M_SQRT2 / ma, sb = M_SQRT2 / mb;
  const bool valid = cnt >= smin && ma > 0 && mb > 0 && isfinite(sa) && isfinite(sb);
  if (valid) {
    for (int i = t; i < n; i += 256) {
      const float2 a = A[i], q = Bp[i];
      float4 o = make_float4(NAN, NAN, NAN, NAN);
      if (finite_row(a.x, a.y, q.x, q.y))
        o = make_float4((float)((a.x - cax) * sa), (float)((a.y - cay) * sa), (float)((q.x - cbx) * sb), (float)((q.y - cby) * sb));
      pts[(long)b * N + i] = o;
    }
  }
  if (t == 0) {
    PairState& S = st[b];
    S.ca[0] = cax; S.ca[1] = cay; S.cb[0] = cbx; S.cb[1] = cby; S.sa = sa; S.sb = sb;
    const double ta = (double)thr * sa, tb = (double)thr * sb;
    S.thr2a = (float)(ta * ta);
    S.thr2b = (float)(tb * tb);
    S.n = n;
    S.valid = valid ? 1 : 0;
    S.best = -1; S.best_h = -1; S.best_root = -1; S.best_min = -1;
    S.needed = max_iters;
    S.rounds = 0;
    S.done = valid ? 0 : 1;
    S.stop = 0;
    S.cand_ok = 0;
    for (int k = 0; k < 9; ++k) { S.cur[k] = 0; S.cand[k] = 0; }
    for (int k = 0; k < 12; ++k) { S.curf[k] = 0; S.candf[k] = 0; }
  }
}

// one thread per (pair, hypothesis of the round); grid B * R / 64
template <int MODEL>
__global__ __launch_bounds__(64) void ransac_hyp_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb, int N,
                                                        const unsigned long long* __restrict__ seeds, const PairState* __restrict__ st,
                                                        int round, double* __restrict__ slot_d, float* __restrict__ slot_f,
                                                        int* __restrict__ slot_n) {
  constexpr int S = Traits<MODEL>::S;
  const int g = blockIdx.x * 64 + threadIdx.x, b = g / R;
  const PairState& P = st[b];
  if (P.done) return;
  const int h = round * R + g % R;
  double m[MAX_ROOTS][9];
  int nm = 0, idx[S];
  if (draw_sample<S>(seeds[b], h, P.n, idx)) {
    double xa[S], ya[S], xb[S], yb[S];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const float2 a = ka[(long)b * N + idx[k]], q = kb[(long)b * N + idx[k]];
      fin &= finite_row(a.x, a.y, q.x, q.y);
      xa[k] = (a.x - P.ca[0]) * P.sa; ya[k] = (a.y - P.ca[1]) * P.sa;
      xb[k] = (q.x - P.cb[0]) * P.sb; yb[k] = (q.y - P.cb[1]) * P.sb;
    }
    if (fin) nm = MODEL == RANSAC_HOMOGRAPHY ? solve_h(xa, ya, xb, yb, m) : solve_f(xa, ya, xb, yb, m);
  }
  slot_n[g] = nm;
#pragma unroll
  for (int r = 0; r < MAX_ROOTS; ++r) {
    float mf[12];
    if (r < nm) {
      to_f32(m[r], mf);
#pragma unroll
      for (int k = 0; k < 9; ++k) slot_d[((long)g * MAX_ROOTS + r) * 9 + k] = m[r][k];
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) mf[k] = 0.f;
    }
    float4* o = reinterpret_cast<float4*>(slot_f + ((long)g * MAX_ROOTS + r) * 12);
    o[0] = make_float4(mf[0], mf[1], mf[2], mf[3]);
    o[1] = make_float4(mf[4], mf[5], mf[6], mf[7]);
    o[2] = make_float4(mf[8], mf[9], mf[10], mf[11]);
  }
}

// one wave per (pair, hypothesis): the hypothesis' models (wave-uniform coefficients) against the pair's points
template <int MODEL>
__global__ __launch_bounds__(256) void ransac_score_kernel(const float4* __restrict__ pts, int N, const PairState* __restrict__ st,
                                                           const float* __restrict__ slot_f, const int* __restrict__ slot_n,
                                                           int* __restrict__ slot_cnt) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = g / R;
  const PairState& P = st[b];
  if (P.done) return;
  const int nm = slot_n[g];
  const float* mf = slot_f + (long)g * MAX_ROOTS * 12;
  const float4* Pp = pts + (long)b * N;
  const int n = P.n;
  const float t2a = P.thr2a, t2b = P.thr2b;
  int c0 = 0, c1 = 0, c2 = 0;
  if (nm > 0) {
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const float4 p = i < n ? Pp[i] : make_float4(NAN, NAN, NAN, NAN);
      c0 += __popcll(__ballot(inlier<MODEL>(mf, p, t2a, t2b)));
      if (MODEL == RANSAC_FUNDAMENTAL) {
        c1 += __popcll(__ballot(inlier<MODEL>(mf + 12, p, t2a, t2b)));
        c2 += __popcll(__ballot(inlier<MODEL>(mf + 24, p, t2a, t2b)));
      }
    }
  }
  if (lane == 0) {
    int* o = slot_cnt + (long)g * MAX_ROOTS;
    o[0] = nm > 0 ? c0 : -1;
    o[1] = nm > 1 ? c1 : -1;
    o[2] = nm > 2 ? c2 : -1;
  }
}

// one workgroup per pair: best (count, lowest slot) of the round, running best, adaptive iteration count, done flag
__global__ __launch_bounds__(256) void ransac_select_kernel(PairState* __restrict__ st, int round, int s, double conf, int max_iters,
                                                            const double* __restrict__ slot_d, const int* __restrict__ slot_cnt) {
  __shared__ int sc[256], si[256];
  const int b = blockIdx.x, t = threadIdx.x;
  PairState& P = st[b];
  if (P.done) return;
  const int* cnt = slot_cnt + (long)b * R * MAX_ROOTS;
  int bc = -1, bi = 0x7fffffff;
  for (int k = t; k < R * MAX_ROOTS; k += 256) {
    const int c = cnt[k];
    if (c > bc) { bc = c; bi = k; }  // k ascends: ties keep the lower slot
  }
  sc[t] = bc;
  si[t] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const int c = sc[t + w], i = si[t + w];
      if (c > sc[t] || (c == sc[t] && i < si[t])) { sc[t] = c; si[t] = i; }
    }
    __syncthreads();
  }
  if (t == 0) {
    const int c = sc[0], k = si[0];
    if (c > P.best) {  // strictly: an earlier round's model keeps a tie
      P.best = c;
      P.best_min = c;
      P.best_h = round * R + k / MAX_ROOTS;
      P.best_root = k % MAX_ROOTS;
      const double* m = slot_d + ((long)b * R * MAX_ROOTS + k) * 9;
      for (int q = 0; q < 9; ++q) P.cur[q] = m[q];
      to_f32(P.cur, P.curf);
      P.needed = update_num_iters(conf, (double)c / P.n, s, max_iters);
    }
    P.rounds = round + 1;
    const long drawn = (long)(round + 1) * R;
    P.done = drawn >= (long)min(max_iters, P.needed) ? 1 : 0;
  }
}

// mask[b, i] = inlier of the current model (rows beyond counts[b], and pairs without a model: 0); grid (ceil(N / 256), B)
template <int MODEL>
__global__ __launch_bounds__(256) void ransac_mask_kernel(const float4* __restrict__ pts, int N, const PairState* __restrict__ st,
                                                          unsigned char* __restrict__ mask) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const PairState& P = st[b];
  bool in = false;
  if (P.best > 0 && i < P.n) in = inlier<MODEL>(P.curf, pts[(long)b * N + i], P.thr2a, P.thr2b);
  mask[(long)b * N + i] = in ? 1 : 0;
}

// ---- refinement: smallest eigenvector of a symmetric PSD matrix by one-sided (Hestenes) Jacobi on one wave.  Lane j < NC
// holds column j of M and of V; the P - 1 rounds of the circle method pair every column with every other once per sweep.
template <int NC, int P>
__device__ void jacobi_min_vec(double (&a)[NC], double (&v)[NC], int lane, double (&out)[NC]) {
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    bool rot = false;
    for (int r = 0; r < P - 1; ++r) {
      int pt = lane;
      if (lane < P) pt = lane == P - 1 ? r : lane == r ? P - 1 : ((2 * r - lane) % (P - 1) + (P - 1)) % (P - 1);
      double pa[NC], pv[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) { pa[k] = __shfl(a[k], pt); pv[k] = __shfl(v[k], pt); }
      const bool lo = lane < pt;
      double al = 0, be = 0, ga = 0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const double ap = lo ? a[k] : pa[k], aq = lo ? pa[k] : a[k];
        al += ap * ap;
        be += aq * aq;
        ga += ap * aq;
      }
      if (pt != lane && fabs(ga) > JACOBI_TOL * sqrt(al * be)) {
        const double z = (be - al) / (2 * ga);
        const double tn = copysign(1.0, z) / (fabs(z) + sqrt(1 + z * z));
        const double c = 1 / sqrt(1 + tn * tn), s = c * tn;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          const double ap = lo ? a[k] : pa[k], aq = lo ? pa[k] : a[k];
          const double vp = lo ? v[k] : pv[k], vq = lo ? pv[k] : v[k];
          a[k] = lo ? c * ap - s * aq : s * ap + c * aq;
          v[k] = lo ? c * vp - s * vq : s * vp + c * vq;
        }
        rot = true;
      }
    }
    if (!__any(rot)) break;
  }
  // column norms of M V are the eigenvalues: the smallest one's column of V (lowest lane on ties)
  double nrm = 0;
#pragma unroll
  for (int k = 0; k < NC; ++k) nrm += a[k] * a[k];
  if (lane >= NC) nrm = INFINITY;
  int bl = lane;
  for (int off = 32; off > 0; off >>= 1) {
    const double on = __shfl_xor(nrm, off);
    const int ol = __shfl_xor(bl, off);
    if (on < nrm || (on == nrm && ol < bl)) { nrm = on; bl = ol; }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) out[k] = __shfl(v[k], bl);
}

// one workgroup per pair: least-squares refit on the current mask (normalised DLT / normalised 8-point + rank 2)
template <int MODEL>
__global__ __launch_bounds__(256) void ransac_refit_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb, int N,
                                                           PairState* __restrict__ st, const unsigned char* __restrict__ mask) {
  __shared__ double red[4][45];
  __shared__ double M[9][9];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  PairState& P = st[b];
  if (P.stop) return;
  if (P.best < Traits<MODEL>::REFIT_MIN) {
    if (t == 0) { P.stop = 1; P.cand_ok = 0; }
    return;
  }
  double acc[45];
#pragma unroll
  for (int e = 0; e < 45; ++e) acc[e] = 0;
  const double cax = P.ca[0], cay = P.ca[1], cbx = P.cb[0], cby = P.cb[1], sa = P.sa, sb = P.sb;
  for (int i = t; i < P.n; i += 256) {
    if (!mask[(long)b * N + i]) continue;
    const float2 a = ka[(long)b * N + i], q = kb[(long)b * N + i];
    const double x = (a.x - cax) * sa, y = (a.y - cay) * sa, u = (q.x - cbx) * sb, v = (q.y - cby) * sb;
    if (MODEL == RANSAC_HOMOGRAPHY) {
      const double r1[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, -u};
      const double r2[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, -v};
      int e = 0;
#pragma unroll
      for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int q2 = p; q2 < 9; ++q2, ++e) acc[e] += r1[p] * r1[q2] + r2[p] * r2[q2];
    } else {
      const double r1[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1};
      int e = 0;
#pragma unroll
      for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int q2 = p; q2 < 9; ++q2, ++e) acc[e] += r1[p] * r1[q2];
    }
  }
#pragma unroll
  for (int e = 0; e < 45; ++e) {
    double s = acc[e];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) red[wave][e] = s;
  }
  __syncthreads();
  if (t < 45) {
    int p = 0, e = t;
    while (e >= 9 - p) { e -= 9 - p; ++p; }
    const int q2 = p + e;
    const double s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    M[p][q2] = s;
    M[q2][p] = s;
  }
  __syncthreads();
  if (wave != 0) return;
  double col[9], vv[9], h[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    col[k] = lane < 9 ? M[k][lane] : 0.0;
    vv[k] = lane == k ? 1.0 : 0.0;
  }
  jacobi_min_vec<9, 10>(col, vv, lane, h);
  if (MODEL == RANSAC_FUNDAMENTAL) {  // rank 2: F - (F v)(v^T), v the smallest right singular vector (eigenvector of F^T F)
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

// one wave per pair: re-score the candidate; keep it if its count is not lower, else stop refining
template <int MODEL>
__global__ __launch_bounds__(64) void ransac_accept_kernel(const float4* __restrict__ pts, int N, PairState* __restrict__ st) {
  const int b = blockIdx.x, lane = threadIdx.x;
  PairState& P = st[b];
  if (P.stop || !P.cand_ok) return;
  const int c = wave_count<MODEL>(P.candf, pts + (long)b * N, P.n, P.thr2a, P.thr2b, lane);
  if (lane == 0) {
    if (c >= P.best) {
      P.best = c;
      for (int k = 0; k < 9; ++k) P.cur[k] = P.cand[k];
      for (int k = 0; k < 12; ++k) P.curf[k] = P.candf[k];
    } else {
      P.stop = 1;
    }
    P.cand_ok = 0;
  }
}

__device__ __forceinline__ void mat3(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// one thread per pair: de-normalise (H = Tb^-1 H_n Ta, F = Tb^T F_n Ta), scale, ok, info
__global__ __launch_bounds__(64) void ransac_finish_kernel(int model, int B, const PairState* __restrict__ st, double* __restrict__ out,
                                                           unsigned char* __restrict__ ok, int* __restrict__ info) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const PairState& P = st[b];
  const bool good = P.valid && P.best > 0;
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (good) {
    const double ta[9] = {P.sa, 0, -P.sa * P.ca[0], 0, P.sa, -P.sa * P.ca[1], 0, 0, 1};
    double l[9], tmp[9];
    if (model == RANSAC_HOMOGRAPHY) {
      const double tbi[9] = {1 / P.sb, 0, P.cb[0], 0, 1 / P.sb, P.cb[1], 0, 0, 1};
      for (int k = 0; k < 9; ++k) l[k] = tbi[k];
    } else {
      const double tbt[9] = {P.sb, 0, 0, 0, P.sb, 0, -P.sb * P.cb[0], -P.sb * P.cb[1], 1};
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
  for (int k = 0; k < 9; ++k) out[(long)b * 9 + k] = m[k];
  ok[b] = good ? 1 : 0;
  int* o = info + (long)b * RANSAC_INFO;
  o[0] = P.rounds;
  o[1] = P.best_h;
  o[2] = P.best_root;
  o[3] = P.best_min;
  o[4] = P.best;
  o[5] = P.valid;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carve {
  PairState* st;
  float4* pts;
  double* slot_d;
  float* slot_f;
  int *slot_n, *slot_cnt;
  size_t bytes;
};

Carve carve(void* ws, int B, int N) {
  Carve c;
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  c.st = reinterpret_cast<PairState*>(p + o); o = align256(o + sizeof(PairState) * B);
  c.pts = reinterpret_cast<float4*>(p + o); o = align256(o + sizeof(float4) * (size_t)B * N);
  c.slot_d = reinterpret_cast<double*>(p + o); o = align256(o + sizeof(double) * 9 * MAX_ROOTS * (size_t)B * R);
  c.slot_f = reinterpret_cast<float*>(p + o); o = align256(o + sizeof(float) * 12 * MAX_ROOTS * (size_t)B * R);
  c.slot_n = reinterpret_cast<int*>(p + o); o = align256(o + sizeof(int) * (size_t)B * R);
  c.slot_cnt = reinterpret_cast<int*>(p + o); o = align256(o + sizeof(int) * MAX_ROOTS * (size_t)B * R);
  c.bytes = o + 256;  // slack: the caller's base need not be 256-aligned
  return c;
}

template <int MODEL>
int launch(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B, int N, float thr,
           double conf, int max_iters, int refine, double* out_model, unsigned char* out_mask, unsigned char* out_ok, int* out_info,
           void* ws, hipStream_t s) {
  const uintptr_t base = (reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255;
  const Carve c = carve(reinterpret_cast<void*>(base), B, N);
  const float2* ka = reinterpret_cast<const float2*>(kpts_a);
  const float2* kb = reinterpret_cast<const float2*>(kpts_b);
  constexpr int S = Traits<MODEL>::S;
  hipLaunchKernelGGL(ransac_norm_kernel, dim3(B), dim3(256), 0, s, ka, kb, counts, N, S, thr, max_iters, c.st, c.pts);
  ROMA_LAUNCH_CHECK();
  const int rounds = (max_iters + R - 1) / R;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(ransac_hyp_kernel<MODEL>, dim3(B * R / 64), dim3(64), 0, s, ka, kb, N, seeds, c.st, r, c.slot_d, c.slot_f,
                       c.slot_n);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_score_kernel<MODEL>, dim3(B * R / 4), dim3(256), 0, s, c.pts, N, c.st, c.slot_f, c.slot_n, c.slot_cnt);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_select_kernel, dim3(B), dim3(256), 0, s, c.st, r, S, conf, max_iters, c.slot_d, c.slot_cnt);
    ROMA_LAUNCH_CHECK();
  }
  const dim3 mgrid((N + 255) / 256, B);
  if (refine) {
    for (int it = 0; it < REFINE_ITERS; ++it) {
      hipLaunchKernelGGL(ransac_mask_kernel<MODEL>, mgrid, dim3(256), 0, s, c.pts, N, c.st, out_mask);
      ROMA_LAUNCH_CHECK();
      hipLaunchKernelGGL(ransac_refit_kernel<MODEL>, dim3(B), dim3(256), 0, s, ka, kb, N, c.st, out_mask);
      ROMA_LAUNCH_CHECK();
      hipLaunchKernelGGL(ransac_accept_kernel<MODEL>, dim3(B), dim3(64), 0, s, c.pts, N, c.st);
      ROMA_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(ransac_mask_kernel<MODEL>, mgrid, dim3(256), 0, s, c.pts, N, c.st, out_mask);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(ransac_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, MODEL, B, c.st, out_model, out_ok, out_info);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace

size_t ransac_workspace_bytes(int B, int N) { return B > 0 && N > 0 ? carve(nullptr, B, N).bytes : 0; }

int ransac_launch(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B,
                  int N, float threshold, double confidence, int max_iters, int refine, double* out_model, unsigned char* out_mask,
                  unsigned char* out_ok, int* out_info, void* ws, size_t ws_bytes, hipStream_t s) {
  ROMA_REQUIRE(model == RANSAC_HOMOGRAPHY || model == RANSAC_FUNDAMENTAL, "ransac: model must be 0 (homography) or 1 (fundamental)");
  ROMA_REQUIRE(kpts_a && kpts_b && seeds && out_model && out_mask && out_ok && out_info && ws, "ransac: null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16), "ransac: need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(max_iters > 0, "ransac: max_iters must be positive");
  ROMA_REQUIRE(threshold > 0 && isfinite(threshold), "ransac: threshold must be positive and finite");
  ROMA_REQUIRE(confidence >= 0 && confidence <= 1, "ransac: confidence must lie in [0, 1]");
  ROMA_REQUIRE(ws_bytes >= ransac_workspace_bytes(B, N), "ransac: workspace too small (roma_op_ransac_workspace)");
  return model == RANSAC_HOMOGRAPHY
             ? launch<RANSAC_HOMOGRAPHY>(kpts_a, kpts_b, counts, seeds, B, N, threshold, confidence, max_iters, refine, out_model,
                                         out_mask, out_ok, out_info, ws, s)
             : launch<RANSAC_FUNDAMENTAL>(kpts_a, kpts_b, counts, seeds, B, N, threshold, confidence, max_iters, refine, out_model,
                                          out_mask, out_ok, out_info, ws, s);
}

}  // namespace roma
