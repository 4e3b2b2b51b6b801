// Bundle adjustment on the device: the cameras (R_i, t_i), x_cam = R_i X + t_i, and the points X_j of B independent problems
// refined together on the reprojection error - the closing step after estimate_pose / triangulate / estimate_absolute_pose,
// which each fit one side with the other held.  tools/bundle_ref.py restates this file in numpy float64 and is the oracle of
// the GPU tests.  lm_fit.h supplies the constants, the truncated cost, the accept / reject / stop rules and the fixed-order
// reductions; the loop is written out here because the state (up to 8 cameras and N points) does not fit lm_fit's registers.
//
// Problem b: V views, counts[b] points.  Row (i, j): the observation of point j in view i (both pixel coordinates finite),
// residual e = p_xy / z - x_n with p = R_i X_j + t_i and x_n = ((u - cx_i) / fx_i, (v - cy_i) / fy_i); active when z > 0 and
// |e|^2 < thr_i^2, thr_i = thr / ((fx_i + fy_i) / 2).  cost = sum over the rows of min(|e|^2, thr_i^2) (a row that is not
// active costs thr_i^2, nothing with thr = inf).  A point beyond counts[b], with a non-finite start or with fewer than two
// observations is not part of the problem: no rows, no cost, returned as it came.
//
// One step at damping lambda (ba_build, ba_factor, ba_trial):
//   points   V_j = sum_i Jp^T Jp, g_j = sum_i Jp^T e over the active rows of point j (Jp = de / dX, 2 x 3); the point is frozen
//            for the step (dX = 0, its rows in the cost but not in the normal equations) with fewer than two active rows or
//            when the Cholesky factor of V_j + lambda diag V_j has a pivot not above LM_PIVOT_REL x its largest diagonal entry;
//            else Vi_j = (V_j + lambda diag V_j)^-1 goes to the workspace
//   cameras  U_i = sum_j Jc^T Jc, g_i = sum_j Jc^T e (Jc = de / d(w, dt), 2 x 6) and the Schur terms: with W_ij = Jc^T Jp,
//            W_ij Vi_j W_kj^T = Jc_i^T (Jp_i Vi_j Jp_k^T) Jc_k - a 2 x 2 matrix between the two camera Jacobians - and
//            W_ij Vi_j g_j = Jc_i^T (Jp_i Vi_j g_j), so S = U + lambda diag U - sum_j W_j Vi_j W_j^T and its right side
//            -(g_c - sum_j W_j Vi_j g_j) need no 6 x 3 block.  A parameter that is held or whose entry of diag U is not
//            positive gets a unit row and a zero right side: its delta is exactly 0
//   solve    S (6V x 6V, at most 48 x 48) by Cholesky in LDS, right-looking, with the pivot test on the free rows; forward
//            and backward substitution by one wave
//   points   dX_j = Vi_j (-g_j - sum_i W_ij^T dc_i), the trial state, |step|^2 and the trial cost in one pass
// The fit stops as lm_fit does: max_steps accepted steps, |step| < LM_STEP_TOL, LM_RETRIES failed retries, a failed pivot of
// S, no free parameter, or fewer active residuals (two per row) than free parameters.  Every solve, a retry included, builds
// the normal equations anew: which points are frozen depends on lambda.
//
// One workgroup of LM_THREADS per problem; points are strided over the threads.  Every camera block is a sum over points:
// each thread adds its points in ascending order into registers (33 sums for a view's diagonal block, diag U and gradient, 36
// for a pair of views), lm_exchange adds the lanes by the xor butterfly and the waves in order.  The sums of one view or one pair
// of views are one pass over the points, V (V + 1) / 2 + 2 passes per step; a pass recomputes the two rows' Jacobians from the
// point (3 doubles), Vi_j and g_j (9) and the cameras in LDS rather than staging W_j and W_j Vi_j (288 doubles a point at V = 8).  No
// atomics; the order of every sum depends on LM_THREADS alone.
#include "../../include/roma_hip.h"
#include "lm_fit.h"

namespace roma {
namespace {

constexpr int ROMA_BA_MAX_VIEWS = 8;   // views of one problem: the reduced camera system is at most 48 x 48
constexpr int BUNDLE_ADJUST_INFO = 6;  // ints per problem in roma_op_bundle_adjust's out_info
constexpr int BA_V = ROMA_BA_MAX_VIEWS, BA_NS = 6 * BA_V;  // views, rows of S
constexpr int BA_CAM = 12, BA_VW = 5;                      // doubles of a camera (R row-major, t) and of a view (fx, fy, cx, cy, thr^2)
constexpr int BA_DIAG = 33, BA_PAIR = 36;                  // sums of a view's pass (block of S 21, diag U 6, reduced gradient 6) and of a pair's
constexpr int BA_BLK = 9;                                  // doubles of a point's block in the workspace: Vi_j (6), g_j (3)

struct BaCarve {
  double *cur, *trial;  // [B][N][3] points: current and trial
  double* blk;          // [B][N][9] (V_j + lambda diag V_j)^-1 (upper triangle), then g_j
  int* flag;            // [B][N] 0: not part of the problem, 1: frozen for the step, 2: adjusted
  size_t bytes;
};

BaCarve ba_carve(Workspace256 ws, int B, int N) {
  BaCarve c;
  const size_t bn = (size_t)B * N;
  c.cur = ws.take<double>(3 * bn);
  c.trial = ws.take<double>(3 * bn);
  c.blk = ws.take<double>(BA_BLK * bn);
  c.flag = ws.take<int>(bn);
  c.bytes = ws.bytes();
  return c;
}

struct BaMem {         // the problem's arrays in global memory
  const float2* kp;    // [V][N]
  double *cur, *trial; // [N][3]
  double* blk;         // [N][BA_BLK]
  int* flag;           // [N]
};

struct BaCtx {
  int V, N, n;         // views, points per problem in memory, points of this problem
  // LDS
  const BaMem* mem;    // the two point buffers of mem->cur / trial swap with cs, see ba_mem
  double* cam;         // [2][BA_V][BA_CAM]: the current and the trial cameras
  const double* vw;    // [BA_V][BA_VW]
  const int* hold;     // [BA_NS]
  double *S, *rhs, *Ld, *dsol, *udiag;
  int* freep;
  double* shx;         // [LM_WAVES][BA_PAIR]
  int* shc;
};

struct BaEnd {  // what only the end of the kernel reads
  const double *pts_in, *R_in, *t_in;
  double *out_pts, *out_R, *out_t, *out_cost;
  unsigned char* mask;
  int* out_info;
};

struct BaStat {  // what the loop leaves for the end
  double cost0;
  int fitted, nadj, nfree;
};

struct BaObs {
  double e[2], q[3], iz, ax, ay, r2;
};

__device__ __forceinline__ bool ba_seen(float2 k) { return isfinite(k.x) && isfinite(k.y); }

// row of the point X in the camera c at the pixel k of the view w: true when the row is active
__device__ __forceinline__ bool ba_residual(const double* c, const double* w, const double (&X)[3], float2 k, BaObs& o) {
  const double x0 = ((double)k.x - w[2]) / w[0], x1 = ((double)k.y - w[3]) / w[1];
  double p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o.q[i] = (c[3 * i] * X[0] + c[3 * i + 1] * X[1]) + c[3 * i + 2] * X[2];
    p[i] = o.q[i] + c[9 + i];
  }
  o.iz = 1.0 / p[2];
  o.ax = p[0] * o.iz;
  o.ay = p[1] * o.iz;
  o.e[0] = o.ax - x0;
  o.e[1] = o.ay - x1;
  o.r2 = p[2] > 0 ? o.e[0] * o.e[0] + o.e[1] * o.e[1] : NAN;
  return o.r2 < w[4];  // false for NaN
}

// what a row adds to the cost
__device__ __forceinline__ double ba_term(bool act, const BaObs& o, const double* w) { return act ? o.r2 : (isfinite(w[4]) ? w[4] : 0.0); }

// de / d(w, dt): dp = e_k x q for the rotation about e_k, e_k for dt_k (AbsPoseFit::jacobian)
__device__ __forceinline__ void ba_jac_cam(const BaObs& o, double (&J)[2][6]) {
  const double* q = o.q;
  const double iz = o.iz, ax = o.ax, ay = o.ay;
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

// de / dX: dp = R e_k
__device__ __forceinline__ void ba_jac_pt(const double* c, const BaObs& o, double (&J)[2][3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    J[0][k] = (c[k] - o.ax * c[6 + k]) * o.iz;
    J[1][k] = (c[3 + k] - o.ay * c[6 + k]) * o.iz;
  }
}

// A = Vi Jp^T (3 x 2), Vi the upper triangle (00, 01, 02, 11, 12, 22)
__device__ __forceinline__ void ba_vi_jpt(const double (&vi)[6], const double (&Jp)[2][3], double (&A)[3][2]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    A[0][r] = (vi[0] * Jp[r][0] + vi[1] * Jp[r][1]) + vi[2] * Jp[r][2];
    A[1][r] = (vi[1] * Jp[r][0] + vi[3] * Jp[r][1]) + vi[4] * Jp[r][2];
    A[2][r] = (vi[2] * Jp[r][0] + vi[4] * Jp[r][1]) + vi[5] * Jp[r][2];
  }
}

template <int NK>
__device__ __forceinline__ void ba_load(const double* a, double (&x)[NK]) {
#pragma unroll
  for (int k = 0; k < NK; ++k) x[k] = a[k];
}

// A value that every thread of the workgroup holds with the same bits (a total read back from LDS), as a scalar: the loop's
// decisions then are scalar branches and its state lives in SGPRs, not in 256 copies per wave
__device__ __forceinline__ int ba_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double ba_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// The problem's arrays for a pass, with the current points in buffer cs.  They are read from LDS where they are used: held
// across the loop they would take the SGPRs the passes need.
__device__ __forceinline__ BaMem ba_mem(const BaCtx& x, int cs) {
  BaMem m = *x.mem;
  if (cs) {
    double* p = m.cur;
    m.cur = m.trial;
    m.trial = p;
  }
  return m;
}

// threadIdx.x, opaque to the optimiser: a predicate on it (t < 21, t == j ...) is then computed where it is used; taken from
// threadIdx.x itself it is hoisted out of the fit's loop and holds an SGPR pair across every pass
__device__ __forceinline__ int ba_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// the points' pass of a step: V_j, g_j, the frozen points, Vi_j and g_j to the workspace.  Returns the cost of the state;
// nact: active rows, nadj: points adjusted, nres: active rows of the adjusted points
__device__ __forceinline__ double ba_points(const BaCtx& x, const BaMem& m, const double* cam, double lam, int& nact, int& nadj, int& nres) {
  double s[3] = {0.0, 0.0, 0.0};  // cost, points adjusted, their active rows (integers are exact in a double)
  int cnt = 0;
#pragma unroll 1
  for (int j = threadIdx.x; j < x.n; j += LM_THREADS) {
    if (!m.flag[j]) continue;
    double X[3], Vj[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gj[3] = {0.0, 0.0, 0.0};
    ba_load(m.cur + 3 * j, X);
    int na = 0;
#pragma unroll 1
    for (int i = 0; i < x.V; ++i) {
      const float2 k = m.kp[i * x.N + j];
      if (!ba_seen(k)) continue;
      const double* c = cam + i * BA_CAM;
      const double* w = x.vw + i * BA_VW;
      BaObs o;
      const bool act = ba_residual(c, w, X, k, o);
      s[0] = s[0] + ba_term(act, o, w);
      if (act) {
        double Jp[2][3];
        ba_jac_pt(c, o, Jp);
        int q = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
          for (int b = a; b < 3; ++b) {
            Vj[q] = Vj[q] + (Jp[0][a] * Jp[0][b] + Jp[1][a] * Jp[1][b]);
            ++q;
          }
          gj[a] = gj[a] + (Jp[0][a] * o.e[0] + Jp[1][a] * o.e[1]);
        }
        ++na;
      }
    }
    cnt += na;
    // Cholesky of V_j + lambda diag V_j, its inverse L^-T L^-1
    const double d0 = Vj[0] + lam * Vj[0], d1 = Vj[3] + lam * Vj[3], d2 = Vj[5] + lam * Vj[5];
    const double piv = LM_PIVOT_REL * fmax(fmax(d0, d1), d2);
    bool pd = d0 > piv;
    const double l00 = sqrt(d0), l10 = Vj[1] / l00, l20 = Vj[2] / l00;
    const double p1 = d1 - l10 * l10;
    pd = pd && p1 > piv;
    const double l11 = sqrt(p1), l21 = (Vj[4] - l20 * l10) / l11;
    const double p2 = (d2 - l20 * l20) - l21 * l21;
    pd = pd && p2 > piv;
    const double l22 = sqrt(p2);
    const bool adj = na >= 2 && pd;
    m.flag[j] = adj ? 2 : 1;
    if (adj) {
      const double a = 1.0 / l00, c = 1.0 / l11, f = 1.0 / l22;
      const double b = (0.0 - (l10 * a)) * c, e = (0.0 - (l21 * c)) * f, d = (0.0 - (l20 * a + l21 * b)) * f;
      const double vi[6] = {(a * a + b * b) + d * d, b * c + d * e, d * f, c * c + e * e, e * f, f * f};
      double* blk = m.blk + BA_BLK * j;
#pragma unroll
      for (int k = 0; k < 6; ++k) blk[k] = vi[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) blk[6 + k] = gj[k];
      s[1] = s[1] + 1.0;
      s[2] = s[2] + (double)na;
    }
  }
  lm_reduce(s, cnt, x.shx, x.shc);
  nact = ba_uniform(cnt);
  nadj = ba_uniform((int)s[1]);
  nres = ba_uniform((int)s[2]);
  return ba_uniform(s[0]);
}

// the active row of the adjusted point j in view i, if there is one: its residual and both Jacobians
__device__ __forceinline__ bool ba_row(const BaCtx& x, const BaMem& m, const double* cam, int i, int j, const double (&X)[3], BaObs& o, double (&Jc)[2][6],
                                       double (&Jp)[2][3]) {
  const float2 k = m.kp[i * x.N + j];
  if (!ba_seen(k)) return false;
  const double* c = cam + i * BA_CAM;
  if (!ba_residual(c, x.vw + i * BA_VW, X, k, o)) return false;
  ba_jac_cam(o, Jc);
  ba_jac_pt(c, o, Jp);
  return true;
}

// view i: U_i - W_i Vi W_i^T (lower triangle), diag U_i and g_i - W_i Vi g into S, udiag and rhs.  With M = Jp Vi Jp^T the
// point adds Jc^T (Jc - M Jc): its share of U_i and of the Schur term in one product.
__device__ __forceinline__ void ba_view(const BaCtx& x, const BaMem& m, const double* cam, double lam, int i) {
  double acc[BA_DIAG];
#pragma unroll
  for (int k = 0; k < BA_DIAG; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (int j = threadIdx.x; j < x.n; j += LM_THREADS) {
    if (m.flag[j] != 2) continue;
    double X[3], Jc[2][6], Jp[2][3];
    ba_load(m.cur + 3 * j, X);
    BaObs o;
    if (!ba_row(x, m, cam, i, j, X, o, Jc, Jp)) continue;
    double vi[6], g[3], A[3][2], M[2][2], D[2][6], h[2];
    ba_load(m.blk + BA_BLK * j, vi);
    ba_load(m.blk + BA_BLK * j + 6, g);
    ba_vi_jpt(vi, Jp, A);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int s = 0; s < 2; ++s) M[r][s] = (Jp[r][0] * A[0][s] + Jp[r][1] * A[1][s]) + Jp[r][2] * A[2][s];
      h[r] = o.e[r] - ((A[0][r] * g[0] + A[1][r] * g[1]) + A[2][r] * g[2]);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int b = 0; b < 6; ++b) D[r][b] = Jc[r][b] - (M[r][0] * Jc[0][b] + M[r][1] * Jc[1][b]);
    int q = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        acc[q] = acc[q] + (Jc[0][a] * D[0][b] + Jc[1][a] * D[1][b]);
        ++q;
      }
      acc[21 + a] = acc[21 + a] + (Jc[0][a] * Jc[0][a] + Jc[1][a] * Jc[1][a]);
      acc[27 + a] = acc[27 + a] + (Jc[0][a] * h[0] + Jc[1][a] * h[1]);
    }
  }
  lm_exchange(acc, 0, x.shx, x.shc);
  const int e = ba_tid();
  if (e < 21) {
    int a = 0, b = e;  // entry e of the lower triangle, row-major
    while (b > a) {
      b -= a + 1;
      ++a;
    }
    const double U = a == b ? lm_total_of<BA_DIAG>(x.shx, 21 + a) : 0.0;
    x.S[(6 * i + a) * BA_NS + 6 * i + b] = lm_total_of<BA_DIAG>(x.shx, e) + lam * U;
    if (a == b) x.udiag[6 * i + a] = U;
  } else if (e < 27) {
    x.rhs[6 * i + e - 21] = 0.0 - lm_total_of<BA_DIAG>(x.shx, 6 + e);
  }
}

// views i < k: the block (k, i) of S, -W_k Vi W_i^T = -Jc_k^T (Jp_k Vi Jp_i^T) Jc_i
__device__ __forceinline__ void ba_pair(const BaCtx& x, const BaMem& m, const double* cam, int i, int k) {
  double acc[BA_PAIR];
#pragma unroll
  for (int q = 0; q < BA_PAIR; ++q) acc[q] = 0.0;
#pragma unroll 1
  for (int j = threadIdx.x; j < x.n; j += LM_THREADS) {
    if (m.flag[j] != 2) continue;
    double X[3], Ji[2][6], Pi[2][3], Jk[2][6], Pk[2][3];
    ba_load(m.cur + 3 * j, X);
    BaObs oi, ok;
    if (!ba_row(x, m, cam, i, j, X, oi, Ji, Pi) || !ba_row(x, m, cam, k, j, X, ok, Jk, Pk)) continue;
    double vi[6], A[3][2], M[2][2], Z[2][6];
    ba_load(m.blk + BA_BLK * j, vi);
    ba_vi_jpt(vi, Pi, A);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int s = 0; s < 2; ++s) M[r][s] = (Pk[r][0] * A[0][s] + Pk[r][1] * A[1][s]) + Pk[r][2] * A[2][s];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int b = 0; b < 6; ++b) Z[r][b] = 0.0 - (M[r][0] * Ji[0][b] + M[r][1] * Ji[1][b]);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) acc[6 * a + b] = acc[6 * a + b] + (Jk[0][a] * Z[0][b] + Jk[1][a] * Z[1][b]);
  }
  lm_exchange(acc, 0, x.shx, x.shc);
  const int e = ba_tid();
  if (e < BA_PAIR) x.S[(6 * k + e / 6) * BA_NS + 6 * i + e % 6] = lm_total_of<BA_PAIR>(x.shx, e);
}

// The normal equations of the state (cam, m.cur) at lam: the points' blocks in the workspace, S and rhs in LDS with the unit
// rows of the parameters that do not move.  Returns the cost; nfree: free camera parameters.
__device__ __forceinline__ double ba_build(const BaCtx& x, int cs, const double* cam, double lam, int& nact, int& nadj, int& nres, int& nfree) {
  const BaMem m = ba_mem(x, cs);
  const double cost = ba_points(x, m, cam, lam, nact, nadj, nres);
#pragma unroll 1
  for (int i = 0; i < x.V; ++i) ba_view(x, m, cam, lam, i);
#pragma unroll 1
  for (int i = 0; i < x.V; ++i)
#pragma unroll 1
    for (int k = i + 1; k < x.V; ++k) ba_pair(x, m, cam, i, k);
  const int n6 = 6 * x.V, t = ba_tid();
  __syncthreads();
  if (t < n6) x.freep[t] = !x.hold[t] && x.udiag[t] > 0 ? 1 : 0;
  __syncthreads();
#pragma unroll 1
  for (int e = t; e < n6 * n6; e += LM_THREADS) {
    const int r = e / n6, c = e % n6;
    if (r >= c && (!x.freep[r] || !x.freep[c])) x.S[r * BA_NS + c] = r == c ? 1.0 : 0.0;
  }
  if (t < n6 && !x.freep[t]) x.rhs[t] = 0.0;
  int nf = 0;
#pragma unroll 1
  for (int a = 0; a < n6; ++a) nf += x.freep[a];
  nfree = ba_uniform(nf);
  __syncthreads();
  return cost;
}

// dc of S dc = rhs into x.dsol; false when a pivot of a free row is not above LM_PIVOT_REL x the largest free diagonal entry.
// S is overwritten by its factor.
__device__ __forceinline__ bool ba_factor(const BaCtx& x) {
  const int n6 = 6 * x.V, t = ba_tid();
  double big = -INFINITY;
#pragma unroll 1
  for (int a = 0; a < n6; ++a) big = x.freep[a] ? fmax(big, x.S[a * BA_NS + a]) : big;
  big = ba_uniform(big);
#pragma unroll 1
  for (int j = 0; j < n6; ++j) {
    const double d = ba_uniform(x.S[j * BA_NS + j]);  // every thread reads the same entry
    if (ba_uniform(x.freep[j]) && !(d > LM_PIVOT_REL * big)) return false;
    const double l = sqrt(d);
    if (t == j) x.Ld[j] = l;
    if (t > j && t < n6) x.S[t * BA_NS + j] = x.S[t * BA_NS + j] / l;
    __syncthreads();
#pragma unroll 1
    for (int e = t; e < n6 * n6; e += LM_THREADS) {
      const int r = e / n6, c = e % n6;
      if (c > j && r >= c) x.S[r * BA_NS + c] = x.S[r * BA_NS + c] - x.S[r * BA_NS + j] * x.S[c * BA_NS + j];
    }
    __syncthreads();
  }
  if (t < 64) {  // one wave: lane r holds row r
    double s = t < n6 ? x.rhs[t] : 0.0;
#pragma unroll 1
    for (int k = 0; k < n6; ++k) {
      const double y = __shfl(s, k, 64) / x.Ld[k];
      if (t == k) s = y;
      else if (t > k && t < n6) s = s - x.S[t * BA_NS + k] * y;
    }
#pragma unroll 1
    for (int k = n6 - 1; k >= 0; --k) {
      const double d = __shfl(s, k, 64) / x.Ld[k];
      if (t == k) s = d;
      else if (t < k) s = s - x.S[k * BA_NS + t] * d;
    }
    if (t < n6) x.dsol[t] = s;
  }
  __syncthreads();
  return true;
}

// camera c moved by d = (w, dt) into o, all in LDS.  Out of line: inlined, the constants of sincos are hoisted out of the
// fit's loop and held across every pass.
__device__ __noinline__ void ba_move_camera(const double* c, const double* d, double* o) {
  if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) {  // a held rotation keeps its bits
    for (int k = 0; k < 9; ++k) o[k] = c[k];
  } else {
    double E[9], Rn[9];
    lm_rodrigues(d[0], d[1], d[2], E);
    mat3(E, c, Rn);
    for (int k = 0; k < 9; ++k) o[k] = Rn[k];
  }
  for (int k = 0; k < 3; ++k) o[9 + k] = d[3 + k] == 0.0 ? c[9 + k] : c[9 + k] + d[3 + k];
}

// The trial state of the step x.dsol from (cam, m.cur): cameras into camn, points into m.trial.  Returns its cost; len2: the
// squared length of the whole step, nact: its active rows.
__device__ __forceinline__ double ba_trial(const BaCtx& x, int cs, const double* cam, double* camn, double& len2, int& nact) {
  const int t = ba_tid();
  if (t < x.V) ba_move_camera(cam + t * BA_CAM, x.dsol + 6 * t, camn + t * BA_CAM);
  __syncthreads();
  const BaMem m = ba_mem(x, cs);
  double s[2] = {0.0, 0.0};  // |dX|^2, cost
  int cnt = 0;
#pragma unroll 1
  for (int j = t; j < x.n; j += LM_THREADS) {
    const int fl = m.flag[j];
    if (!fl) continue;
    double X[3];
    ba_load(m.cur + 3 * j, X);
    if (fl == 2) {
      double w[3] = {0.0, 0.0, 0.0}, vi[6], g[3];
#pragma unroll 1
      for (int i = 0; i < x.V; ++i) {
        double Jc[2][6], Jp[2][3];
        BaObs o;
        if (!ba_row(x, m, cam, i, j, X, o, Jc, Jp)) continue;
        const double* d = x.dsol + 6 * i;
        double u[2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
          u[r] = ((Jc[r][0] * d[0] + Jc[r][1] * d[1]) + (Jc[r][2] * d[2] + Jc[r][3] * d[3])) + (Jc[r][4] * d[4] + Jc[r][5] * d[5]);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = w[k] + (Jp[0][k] * u[0] + Jp[1][k] * u[1]);
      }
      ba_load(m.blk + BA_BLK * j, vi);
      ba_load(m.blk + BA_BLK * j + 6, g);
      const double b0 = (0.0 - g[0]) - w[0], b1 = (0.0 - g[1]) - w[1], b2 = (0.0 - g[2]) - w[2];
      const double dX[3] = {(vi[0] * b0 + vi[1] * b1) + vi[2] * b2, (vi[1] * b0 + vi[3] * b1) + vi[4] * b2,
                            (vi[2] * b0 + vi[4] * b1) + vi[5] * b2};
      s[0] = s[0] + ((dX[0] * dX[0] + dX[1] * dX[1]) + dX[2] * dX[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] = X[k] + dX[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) m.trial[3 * j + k] = X[k];
#pragma unroll 1
    for (int i = 0; i < x.V; ++i) {
      const float2 k = m.kp[i * x.N + j];
      if (!ba_seen(k)) continue;
      const double* w = x.vw + i * BA_VW;
      BaObs o;
      const bool act = ba_residual(camn + i * BA_CAM, w, X, k, o);
      s[1] = s[1] + ba_term(act, o, w);
      cnt += act ? 1 : 0;
    }
  }
  lm_reduce(s, cnt, x.shx, x.shc);
  double dc2 = 0.0;
#pragma unroll 1
  for (int a = 0; a < 6 * x.V; ++a) dc2 = dc2 + x.dsol[a] * x.dsol[a];
  len2 = ba_uniform(dc2 + s[0]);
  nact = ba_uniform(cnt);
  return ba_uniform(s[1]);
}

__global__ __launch_bounds__(LM_THREADS) void bundle_adjust_kernel(
    const double* __restrict__ pts_in, const float2* __restrict__ kpts, const double* __restrict__ K, const double* __restrict__ R_in,
    const double* __restrict__ t_in, const unsigned char* __restrict__ hold, const int* __restrict__ counts,
    const unsigned char* __restrict__ valid, int V, int N, double thr, int max_steps, double* __restrict__ out_pts,
    double* __restrict__ out_R, double* __restrict__ out_t, unsigned char* __restrict__ mask, int* __restrict__ out_info,
    double* __restrict__ out_cost, BaCarve ws) {
  __shared__ double cams[2 * BA_V * BA_CAM];
  __shared__ double vw[BA_V * BA_VW];
  __shared__ double S[BA_NS * BA_NS];
  __shared__ double rhs[BA_NS], Ld[BA_NS], dsol[BA_NS], udiag[BA_NS];
  __shared__ double shx[LM_WAVES * BA_PAIR];
  __shared__ int holdp[BA_NS], freep[BA_NS], shc[LM_WAVES];
  // the arguments of the end wait in LDS: the loop needs the SGPRs they would hold across it
  __shared__ BaEnd endp;
  __shared__ BaMem memp;
  __shared__ BaStat stat;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  const long pb = (long)b * N;  // B * V * N < 2^31 and N <= 2^27: a problem's own indices fit an int
  const BaMem m0 = {kpts + (long)b * V * N, ws.cur + 3 * pb, ws.trial + 3 * pb, ws.blk + BA_BLK * pb, ws.flag + pb};
  if (t == 0) {
    endp = {pts_in, R_in, t_in, out_pts, out_R, out_t, out_cost, mask, out_info};
    memp = m0;
    stat = {NAN, 0, 0, 0};
  }
  BaCtx x;
  x.V = V; x.N = N; x.n = n;
  x.mem = &memp;
  x.cam = cams; x.vw = vw; x.hold = holdp;
  x.S = S; x.rhs = rhs; x.Ld = Ld; x.dsol = dsol; x.udiag = udiag; x.freep = freep; x.shx = shx; x.shc = shc;

#pragma unroll 1
  for (int e = t; e < V * BA_CAM; e += LM_THREADS) {
    const int i = e / BA_CAM, k = e % BA_CAM;
    cams[e] = k < 9 ? R_in[((long)b * V + i) * 9 + k] : t_in[((long)b * V + i) * 3 + k - 9];
  }
  if (t < V) {
    const double* Ki = K ? K + ((long)b * V + t) * 9 : nullptr;
    const double fx = Ki ? Ki[0] : 1.0, fy = Ki ? Ki[4] : 1.0;
    const double tn = Ki ? thr / ((fx + fy) / 2) : thr;
    vw[t * BA_VW] = fx;
    vw[t * BA_VW + 1] = fy;
    vw[t * BA_VW + 2] = Ki ? Ki[2] : 0.0;
    vw[t * BA_VW + 3] = Ki ? Ki[5] : 0.0;
    vw[t * BA_VW + 4] = tn * tn;
  }
  if (t < 6 * V) holdp[t] = hold ? hold[(long)b * V * 6 + t] : 0;
  // the points of the problem: a finite start and at least two observations
#pragma unroll 1
  for (int j = t; j < n; j += LM_THREADS) {
    double X[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = pts_in[(pb + j) * 3 + k];
    int seen = 0;
#pragma unroll 1
    for (int i = 0; i < V; ++i) seen += ba_seen(m0.kp[i * N + j]) ? 1 : 0;
    const bool in = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && seen >= 2;
    m0.flag[j] = in ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) m0.cur[3 * j + k] = X[k];
  }
  __syncthreads();
  bool ok = !valid || valid[b];
#pragma unroll 1
  for (int e = 0; e < V * BA_CAM; ++e) ok = ok && isfinite(cams[e]);
  ok = ba_uniform(ok ? 1 : 0) != 0;

  // lm_fit's loop, one pass of it per solve; every branch is uniform over the workgroup (ba_uniform)
  int cs = 0, steps = 0, evals = 0, nact = 0;
  double cur = NAN, lam = LM_LAMBDA0;
  for (int tr = 0; ok;) {
    const double* cam = cams + cs * BA_V * BA_CAM;
    double* camn = cams + (cs ^ 1) * BA_V * BA_CAM;
    int na, nadj, nres, nfree;
    const double c0 = ba_build(x, cs, cam, lam, na, nadj, nres, nfree);
    const bool can = nfree + 3 * nadj > 0 && 2 * nres >= nfree + 3 * nadj;
    if (t == 0) {
      stat.nadj = nadj;
      stat.nfree = nfree;
    }
    if (evals == 0) {
      cur = c0;
      nact = na;
      evals = 1;
      if (t == 0) {
        stat.cost0 = c0;
        stat.fitted = can ? 1 : 0;
      }
    }
    if (!can || steps >= max_steps || !ba_factor(x)) break;
    double len2;
    const double c = ba_trial(x, cs, cam, camn, len2, na);
    if (sqrt(len2) < LM_STEP_TOL) break;
    ++evals;
    if (c < cur) {
      cs ^= 1;  // the trial cameras and points become the current ones
      cur = c;
      nact = na;
      lam = fmax(lam / 10.0, LM_LAMBDA_MIN);
      tr = 0;
      if (++steps >= max_steps) break;
    } else {
      lam = lam * 10.0;
      if (++tr > LM_RETRIES) break;
    }
  }
  __syncthreads();
  const BaEnd z = endp;
  const bool fitted = stat.fitted != 0;
  const BaMem m = ba_mem(x, cs);
  const double* cam = cams + cs * BA_V * BA_CAM;
  // without an accepted step the input comes back untouched; so does every point that is not part of the problem
#pragma unroll 1
  for (int e = t; e < V * BA_CAM; e += LM_THREADS) {
    const int i = e / BA_CAM, k = e % BA_CAM;
    const long v = (long)b * V + i;
    if (k < 9) z.out_R[v * 9 + k] = steps ? cam[e] : z.R_in[v * 9 + k];
    else z.out_t[v * 3 + k - 9] = steps ? cam[e] : z.t_in[v * 3 + k - 9];
  }
  if (t == 0) {
    int* row = z.out_info + (long)b * BUNDLE_ADJUST_INFO;
    row[0] = steps;
    row[1] = evals;
    row[2] = nact;
    row[3] = stat.nadj;
    row[4] = stat.nfree;
    row[5] = stat.fitted;
    z.out_cost[2 * (long)b] = stat.cost0;
    z.out_cost[2 * (long)b + 1] = cur;
  }
  // the points, and the rows active under the state returned
#pragma unroll 1
  for (int j = t; j < N; j += LM_THREADS) {
    const bool in = j < n && m.flag[j];
    double X[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      X[k] = steps && in ? m.cur[3 * j + k] : z.pts_in[(pb + j) * 3 + k];
      z.out_pts[(pb + j) * 3 + k] = X[k];
    }
#pragma unroll 1
    for (int i = 0; i < V; ++i) {
      bool act = false;
      if (fitted && in) {
        const float2 k = m.kp[i * N + j];
        BaObs o;
        act = ba_seen(k) && ba_residual(cam + i * BA_CAM, vw + i * BA_VW, X, k, o);
      }
      z.mask[((long)b * V + i) * N + j] = act ? 1 : 0;
    }
  }
}

}  // namespace

extern "C" long roma_op_bundle_adjust_workspace(int B, int V, int N) {
  return B > 0 && V > 0 && N > 0 ? ba_carve(Workspace256(), B, N).bytes : 0;
}

extern "C" int roma_op_bundle_adjust(const double* points, const float* kpts, const double* K, const double* R_, const double* t,
                                     const unsigned char* hold, const int* counts, const unsigned char* valid, int B, int V, int N,
                                     double thr, int max_steps, double* out_points, double* out_r, double* out_t, unsigned char* out_mask,
                                     int* out_info, double* out_cost, void* ws, long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(points && kpts && R_ && t && out_points && out_r && out_t && out_mask && out_info && out_cost && ws,
               "bundle_adjust: null pointer");
  ROMA_REQUIRE(V >= 1 && V <= ROMA_BA_MAX_VIEWS, "bundle_adjust: need 1 <= V <= 8 views");
  ROMA_REQUIRE(B > 0 && B <= 65535 && N > 0 && N <= (1 << 27) && (long)B * V * N < (1l << 31),
               "bundle_adjust: need 0 < B <= 65535, 0 < N <= 2^27, B * V * N < 2^31");
  ROMA_REQUIRE(thr > 0, "bundle_adjust: threshold must be positive (+inf: plain least squares)");  // false for NaN
  ROMA_REQUIRE(max_steps >= 0 && max_steps <= (1 << 16), "bundle_adjust: need 0 <= max_steps <= 65536");
  ROMA_REQUIRE(ws_bytes >= (size_t)roma_op_bundle_adjust_workspace(B, V, N), "bundle_adjust: workspace too small");
  const BaCarve c = ba_carve(Workspace256(ws), B, N);
  hipLaunchKernelGGL(bundle_adjust_kernel, dim3(B), dim3(LM_THREADS), 0, s, points, reinterpret_cast<const float2*>(kpts), K, R_, t, hold,
                     counts, valid, V, N, thr, max_steps, out_points, out_r, out_t, out_mask, out_info, out_cost, c);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
