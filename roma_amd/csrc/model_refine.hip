// Nonlinear refinement of a homography or a fundamental matrix on the device: a Levenberg-Marquardt fit to the rows inside
// the threshold under a hard-truncated loss - the forward reprojection error in image B for H (what
// cv2.findHomography(..., RANSAC) ends with) and the Sampson distance for F (what PoseLib's estimate_fundamental ends with).
// It follows roma_op_ransac / roma_op_magsac, whose last step is an algebraic least-squares refit.
// tools/model_refine_ref.py restates this file in numpy float64 expression by expression and is the oracle of the GPU tests.
//
//   coordinates x^ = (x - c) s, Hartley normalisation over the pair's finite rows (centroid to 0, mean distance to sqrt 2, the
//               definition of the RANSAC pipeline; summed here in this kernel's own fixed order); the fit runs on
//               M^ = T_b M T_a^-1 (H) or T_b^-T M T_a^-1 (F) scaled to unit Frobenius norm; residuals are in pixels
//
// The loop - cost, iteration, stopping rules, the reduction and its fixed order - is lm_fit<P> of lm_fit.h, which this file
// shares with pose_refine.hip.  Its policies here:
//
// HomographyFit (8 parameters, two residuals per row): p = H^ (x^, y^, 1), e = ((p_x / p_z - u^) / s_b, (p_y / p_z - v^) / s_b);
//   the entry of the start with the largest magnitude (first maximum, row-major) is held fixed, the other eight are updated
//   additively.
// FundamentalFit (7 parameters, one residual): l = F^ x^_a, k = F^T x^_b, c = x^_b . l,
//   r = c / sqrt(s_b^2 (l_0^2 + l_1^2) + s_a^2 (k_0^2 + k_1^2)); F^ = U diag(1, sigma, 0) V^T with rotations U, V from a
//   one-sided Jacobi SVD of the start (u_2 = u_0 x u_1, v_2 = v_0 x v_1); U <- U exp([a]x), V <- V exp([b]x), sigma <- sigma + d.
//   Every parameter's dF^ is a combination of u_i v_j^T, whose dl = u_i (v_j . x^_a), dk = v_j (u_i . x^_b): the Jacobian needs
//   six dot products per row and no derivative matrices in registers.
//
// model_refine_kernel<P>: one workgroup of LM_THREADS per pair runs the normalisation (summed like the loop's passes: results are
// bit-identical from run to run, independent of B and of the pair's place in the batch), lm_fit<P> and the de-normalisation.
// model_refine_mask_kernel<P>: grid (point blocks, pair): mask = active under the final model.
#include "../../include/roma_hip.h"
#include "geometry.h"
#include "lm_fit.h"  // and through it ransac.h: mat3, finite_row, workspace.h; its fp-contract setting holds here as well

namespace roma {
namespace {

constexpr int MR_SVD_SWEEPS = 20;
constexpr double MR_SVD_TOL = 4 * DBL_EPSILON;

struct MrNorm {
  double ca[2], cb[2], sa, sb;  // x^ = (x - c) * s
};

struct MrState {  // what the fit leaves for the mask kernel
  double m[9];    // final M^
  MrNorm nrm;
  int n, valid;
};

// ------------------------------------------------------------------------------------------------------------ model policies
// The policies of lm_fit.h's loop.  Beside what the loop asks for: init (the state of a unit-norm M^; false if it has none),
// matrix (M^ of a state), matrix_aux (the Aux of an M^: the mask kernel's), left (the left factor of the normalisation or of
// its inverse).
struct NormalisedRows {  // what both have in common: the rows are read through the pair's Hartley normalisation
  using Prep = MrNorm;
  __device__ static LmPoint point(const MrNorm& q, float2 a, float2 b) {
    LmPoint w;
    w.x = (a.x - q.ca[0]) * q.sa;
    w.y = (a.y - q.ca[1]) * q.sa;
    w.u = (b.x - q.cb[0]) * q.sb;
    w.v = (b.y - q.cb[1]) * q.sb;
    return w;
  }
};

struct HomographyFit : NormalisedRows {
  static constexpr int NP = 8, NR = 2, MIN_ROWS = 4;
  struct State { double h[9]; int k0; };
  struct Aux { double m[9], isb; };
  struct Row { double p[3]; };

  __device__ static bool init(const double* mn, State& s) {
    int k0 = 0;
    double big = fabs(mn[0]);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      s.h[k] = mn[k];
      if (fabs(mn[k]) > big) { big = fabs(mn[k]); k0 = k; }
    }
    s.k0 = k0;
    return true;
  }
  __device__ static void matrix_aux(const double* m, const MrNorm& q, Aux& ax) {
#pragma unroll
    for (int k = 0; k < 9; ++k) ax.m[k] = m[k];
    ax.isb = 1.0 / q.sb;
  }
  __device__ static void aux(const State& s, const MrNorm& q, Aux& ax) { matrix_aux(s.h, q, ax); }

  __device__ static double residual(const Aux& ax, const LmPoint& w, Row& r, double (&e)[NR]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) r.p[i] = (ax.m[3 * i] * w.x + ax.m[3 * i + 1] * w.y) + ax.m[3 * i + 2];
    e[0] = (r.p[0] / r.p[2] - w.u) * ax.isb;
    e[1] = (r.p[1] / r.p[2] - w.v) * ax.isb;
    return e[0] * e[0] + e[1] * e[1];
  }

  __device__ static void jacobian(const State& s, const Aux& ax, const LmPoint& w, const Row& r, const double (&e)[NR],
                                  double (&J)[NR][NP]) {
    const double iz = 1.0 / r.p[2];
    const double a = iz * ax.isb;
    const double qx = (r.p[0] * iz) * a, qy = (r.p[1] * iz) * a;
    const double c0 = w.x * a, c1 = w.y * a;
    const double jx[9] = {c0, c1, a, 0.0, 0.0, 0.0, -(qx * w.x), -(qx * w.y), -qx};
    const double jy[9] = {0.0, 0.0, 0.0, c0, c1, a, -(qy * w.x), -(qy * w.y), -qy};
#pragma unroll
    for (int j = 0; j < NP; ++j) {  // the eight columns other than k0, by selects: no indexed registers
      J[0][j] = j >= s.k0 ? jx[j + 1] : jx[j];
      J[1][j] = j >= s.k0 ? jy[j + 1] : jy[j];
    }
  }

  __device__ static void apply(const State& s, const double (&d)[NP], State& o) {
    o.k0 = s.k0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double dk = k == 0 ? d[0] : k == 8 ? d[7] : (k > s.k0 ? d[k - 1] : d[k]);
      o.h[k] = k == s.k0 ? s.h[k] : s.h[k] + dk;
    }
  }
  __device__ static void matrix(const State& s, double* m) {
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = s.h[k];
  }
  // M^ = T_b H T_a^-1; H = T_b^-1 H^ T_a
  __device__ static void left(const MrNorm& q, bool inverse, double* l) {
    const double f[9] = {q.sb, 0, -q.sb * q.cb[0], 0, q.sb, -q.sb * q.cb[1], 0, 0, 1};
    const double i[9] = {1 / q.sb, 0, q.cb[0], 0, 1 / q.sb, q.cb[1], 0, 0, 1};
#pragma unroll
    for (int k = 0; k < 9; ++k) l[k] = inverse ? i[k] : f[k];
  }
};

struct FundamentalFit : NormalisedRows {
  static constexpr int NP = 7, NR = 1, MIN_ROWS = 7;
  struct State { double U[9], V[9], sg; };  // row-major
  struct Aux { double m[9], sa2, sb2; };
  struct Row { double l[2], k[2], den, s; };

  // one-sided Jacobi on the columns of the start (A V = U S; essential.hip's decomposition), singular values descending
  __device__ static bool init(const double* mn, State& st) {
    double a[3][3], v[3][3];  // a[j] = column j
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        a[j][i] = mn[3 * i + j];
        v[j][i] = i == j ? 1.0 : 0.0;
      }
    for (int sweep = 0; sweep < MR_SVD_SWEEPS; ++sweep) {
      bool rot = false;
#pragma unroll
      for (int pq = 0; pq < 3; ++pq) {
        const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
        double al = 0, be = 0, ga = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          al += a[p][k] * a[p][k];
          be += a[q][k] * a[q][k];
          ga += a[p][k] * a[q][k];
        }
        if (fabs(ga) > MR_SVD_TOL * sqrt(al * be)) {
          const double zz = (be - al) / (2 * ga);
          const double tn = copysign(1.0, zz) / (fabs(zz) + sqrt(1 + zz * zz));
          const double c = 1 / sqrt(1 + tn * tn), s = c * tn;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double ap = a[p][k], aq = a[q][k], vp = v[p][k], vq = v[q][k];
            a[p][k] = c * ap - s * aq;
            a[q][k] = s * ap + c * aq;
            v[p][k] = c * vp - s * vq;
            v[q][k] = s * vp + c * vq;
          }
          rot = true;
        }
      }
      if (!rot) break;
    }
    double sg[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) sg[j] = sqrt((a[j][0] * a[j][0] + a[j][1] * a[j][1]) + a[j][2] * a[j][2]);
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
      const int p = pass == 1 ? 1 : 0, q = p + 1;
      if (sg[q] > sg[p]) {
        double t = sg[p]; sg[p] = sg[q]; sg[q] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          t = a[p][k]; a[p][k] = a[q][k]; a[q][k] = t;
          t = v[p][k]; v[p][k] = v[q][k]; v[q][k] = t;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      st.U[3 * k] = a[0][k] / sg[0];
      st.U[3 * k + 1] = a[1][k] / sg[1];
      st.V[3 * k] = v[0][k];
      st.V[3 * k + 1] = v[1][k];
    }
    cross_col(st.U);
    cross_col(st.V);
    st.sg = sg[1] / sg[0];
    return sg[1] > 0 && isfinite(sg[0]);
  }
  __device__ static void cross_col(double* U) {  // column 2 = column 0 x column 1
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
  }

  __device__ static void matrix(const State& s, double* m) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) m[3 * i + j] = s.U[3 * i] * s.V[3 * j] + s.sg * (s.U[3 * i + 1] * s.V[3 * j + 1]);
  }
  __device__ static void matrix_aux(const double* m, const MrNorm& q, Aux& ax) {
#pragma unroll
    for (int k = 0; k < 9; ++k) ax.m[k] = m[k];
    ax.sa2 = q.sa * q.sa;
    ax.sb2 = q.sb * q.sb;
  }
  __device__ static void aux(const State& s, const MrNorm& q, Aux& ax) {
    double m[9];
    matrix(s, m);
    matrix_aux(m, q, ax);
  }

  __device__ static double residual(const Aux& ax, const LmPoint& w, Row& r, double (&e)[NR]) {
    const double* F = ax.m;
    const double l0 = (F[0] * w.x + F[1] * w.y) + F[2], l1 = (F[3] * w.x + F[4] * w.y) + F[5], l2 = (F[6] * w.x + F[7] * w.y) + F[8];
    r.l[0] = l0;
    r.l[1] = l1;
    r.k[0] = (F[0] * w.u + F[3] * w.v) + F[6];
    r.k[1] = (F[1] * w.u + F[4] * w.v) + F[7];
    const double c = (w.u * l0 + w.v * l1) + l2;
    r.den = ax.sb2 * (l0 * l0 + l1 * l1) + ax.sa2 * (r.k[0] * r.k[0] + r.k[1] * r.k[1]);
    r.s = sqrt(r.den);
    e[0] = c / r.s;
    return e[0] * e[0];
  }

  __device__ static void jacobian(const State& st, const Aux& ax, const LmPoint& w, const Row& r, const double (&e)[NR],
                                  double (&J)[NR][NP]) {
    const double inv_s = 1.0 / r.s, inv_den = 1.0 / r.den;
    const double* U = st.U;
    const double* V = st.V;
    double al[3], be[3], Lu[3], Kv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      al[j] = (V[j] * w.x + V[3 + j] * w.y) + V[6 + j];
      be[j] = (U[j] * w.u + U[3 + j] * w.v) + U[6 + j];
      Lu[j] = (r.l[0] * U[j] + r.l[1] * U[3 + j]) * ax.sb2;
      Kv[j] = (r.k[0] * V[j] + r.k[1] * V[3 + j]) * ax.sa2;
    }
    // dr of dF^ = u_i v_j^T
    auto T = [&](int i, int j) { return (be[i] * al[j]) * inv_s - e[0] * ((Lu[i] * al[j] + Kv[j] * be[i]) * inv_den); };
    const double sg = st.sg;
    J[0][0] = sg * T(2, 1);
    J[0][1] = -T(2, 0);
    J[0][2] = T(1, 0) - sg * T(0, 1);
    J[0][3] = sg * T(1, 2);
    J[0][4] = -T(0, 2);
    J[0][5] = T(0, 1) - sg * T(1, 0);
    J[0][6] = T(1, 1);
  }

  __device__ static void apply(const State& s, const double (&d)[NP], State& o) {
    double E[9];
    lm_rodrigues(d[0], d[1], d[2], E);
    mat3(s.U, E, o.U);
    lm_rodrigues(d[3], d[4], d[5], E);
    mat3(s.V, E, o.V);
    o.sg = s.sg + d[6];
  }
  // M^ = T_b^-T F T_a^-1; F = T_b^T F^ T_a
  __device__ static void left(const MrNorm& q, bool inverse, double* l) {
    const double f[9] = {1 / q.sb, 0, 0, 0, 1 / q.sb, 0, q.cb[0], q.cb[1], 1};
    const double i[9] = {q.sb, 0, 0, 0, q.sb, 0, -q.sb * q.cb[0], -q.sb * q.cb[1], 1};
#pragma unroll
    for (int k = 0; k < 9; ++k) l[k] = inverse ? i[k] : f[k];
  }
};

// ------------------------------------------------------------------------------------------------------------ the kernels
// Hartley normalisation of the pair over its finite rows; false if it is not defined
__device__ __forceinline__ bool mr_normalise(const float2* ka, const float2* kb, int n, double* sh, int* shc, MrNorm& q) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    const float2 a = ka[i], b = kb[i];
    if (finite_row(a.x, a.y, b.x, b.y)) {
      s[0] = s[0] + a.x; s[1] = s[1] + a.y; s[2] = s[2] + b.x; s[3] = s[3] + b.y;
      ++cnt;
    }
  }
  lm_reduce(s, cnt, sh, shc);
  const double c = (double)cnt;
  q.ca[0] = s[0] / c; q.ca[1] = s[1] / c; q.cb[0] = s[2] / c; q.cb[1] = s[3] / c;
  double d[2] = {0.0, 0.0};
  int cnt2 = 0;
  for (int i = threadIdx.x; i < n; i += LM_THREADS) {
    const float2 a = ka[i], b = kb[i];
    if (finite_row(a.x, a.y, b.x, b.y)) {
      const double ax = a.x - q.ca[0], ay = a.y - q.ca[1], bx = b.x - q.cb[0], by = b.y - q.cb[1];
      d[0] = d[0] + sqrt(ax * ax + ay * ay);
      d[1] = d[1] + sqrt(bx * bx + by * by);
    }
  }
  lm_reduce(d, cnt2, sh, shc);
  const double ma = d[0] / c, mb = d[1] / c;
  q.sa = M_SQRT2 / ma;
  q.sb = M_SQRT2 / mb;
  return cnt > 0 && ma > 0 && mb > 0 && isfinite(q.sa) && isfinite(q.sb);
}

template <class P>
__global__ __launch_bounds__(LM_THREADS) void model_refine_kernel(const double* __restrict__ M_in, const float2* __restrict__ kpts_a,
                                                                  const float2* __restrict__ kpts_b, const int* __restrict__ counts,
                                                                  const unsigned char* __restrict__ valid, int N, double thr,
                                                                  int max_steps, double* __restrict__ out_M, int* __restrict__ out_info,
                                                                  double* __restrict__ out_cost, MrState* __restrict__ st) {
  __shared__ double shn[LM_WAVES * lm_sums(P::NP)];  // the waves' sums of the normal equations: kept across the retries of a step
  __shared__ double sh[LM_WAVES * 4];    // every other exchange
  __shared__ int shc[LM_WAVES];
  const int b = blockIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  const float2* ka = kpts_a + (long)b * N;
  const float2* kb = kpts_b + (long)b * N;
  // uniform over the workgroup, like every branch below: all threads hold the same values
  bool ok = (!valid || valid[b]) && n >= P::MIN_ROWS;
  MrNorm q;
  typename P::State S;
  double mn[9];
  if (ok) ok = mr_normalise(ka, kb, n, sh, shc, q);
  if (ok) {
    double m[9], l[9], tmp[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      m[k] = M_in[(long)b * 9 + k];
      ok = ok && isfinite(m[k]);
    }
    const double rm[9] = {1 / q.sa, 0, q.ca[0], 0, 1 / q.sa, q.ca[1], 0, 0, 1};
    P::left(q, false, l);
    mat3(l, m, tmp);
    mat3(tmp, rm, mn);
    double f = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) f = f + mn[k] * mn[k];
    f = sqrt(f);
    ok = ok && f > 0 && isfinite(f);
#pragma unroll
    for (int k = 0; k < 9; ++k) mn[k] = mn[k] / f;
    ok = ok && P::init(mn, S);
  }
  LmResult fit = {0, 0, 0, NAN, NAN};
  if (ok) fit = lm_fit<P>(S, q, ka, kb, n, thr * thr, max_steps, shn, sh, shc);
  if (threadIdx.x == 0) {
    MrState& T = st[b];
    T.n = n;
    T.valid = ok ? 1 : 0;
    double out[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = 0.0;
    if (ok) {
      T.nrm = q;
      P::matrix(S, T.m);
      if (fit.steps) {  // the last lines of the RANSAC: de-normalise, [2, 2] = 1 unless it is below 1e-12 of the norm
        const double ta[9] = {q.sa, 0, -q.sa * q.ca[0], 0, q.sa, -q.sa * q.ca[1], 0, 0, 1};
        double l[9], tmp[9];
        P::left(q, true, l);
        mat3(l, T.m, tmp);
        mat3(tmp, ta, out);
        double fro = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) fro = fro + out[k] * out[k];
        fro = sqrt(fro);
        const double sc = fabs(out[8]) >= 1e-12 * fro ? out[8] : fro;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = out[k] / sc;
      }
    }
    // without an accepted step the input comes back untouched (read again: not kept in registers)
    for (int k = 0; k < 9; ++k) out_M[(long)b * 9 + k] = fit.steps ? out[k] : M_in[(long)b * 9 + k];
    out_info[b * 4] = fit.steps;
    out_info[b * 4 + 1] = fit.evals;
    out_info[b * 4 + 2] = fit.nact;
    out_info[b * 4 + 3] = ok ? 1 : 0;
    out_cost[b * 2] = fit.cost0;
    out_cost[b * 2 + 1] = fit.cost;
  }
}

// grid (ceil(N / 256), B): mask[b, i] = active under the final model
template <class P>
__global__ __launch_bounds__(256) void model_refine_mask_kernel(const float2* __restrict__ kpts_a, const float2* __restrict__ kpts_b, int N,
                                                                double thr, const MrState* __restrict__ st,
                                                                unsigned char* __restrict__ mask) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const MrState& S = st[b];
  bool in = false;
  if (S.valid && i < S.n) {
    typename P::Aux ax;
    P::matrix_aux(S.m, S.nrm, ax);
    const LmPoint w = P::point(S.nrm, kpts_a[(long)b * N + i], kpts_b[(long)b * N + i]);
    typename P::Row r;
    double e[P::NR];
    in = P::residual(ax, w, r, e) < thr * thr;
  }
  mask[(long)b * N + i] = in ? 1 : 0;
}

template <class P>
int refine_model_run(const double* M, const float2* ka, const float2* kb, const int* counts, const unsigned char* valid, int B, int N,
                     double thr, int max_steps, double* out_m, unsigned char* out_mask, int* out_info, double* out_cost, MrState* st,
                     hipStream_t s) {
  hipLaunchKernelGGL(model_refine_kernel<P>, dim3(B), dim3(LM_THREADS), 0, s, M, ka, kb, counts, valid, N, thr, max_steps, out_m,
                     out_info, out_cost, st);
  ROMA_LAUNCH_CHECK();
  if (N > 0) {
    hipLaunchKernelGGL(model_refine_mask_kernel<P>, dim3((N + 255) / 256, B), dim3(256), 0, s, ka, kb, N, thr, st, out_mask);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

// the workspace is the pairs' states; returns its bytes
size_t model_refine_carve(Workspace256 ws, int B, MrState*& st) {
  st = ws.take<MrState>(B);
  return ws.bytes();
}

}  // namespace

extern "C" long roma_op_refine_model_workspace(int B, int N) {
  MrState* st;
  return B > 0 && N >= 0 ? model_refine_carve(Workspace256(), B, st) : 0;
}

extern "C" int roma_op_refine_model(int model, const double* M, const float* kpts_a, const float* kpts_b, const int* counts,
                                    const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_m,
                                    unsigned char* out_mask, int* out_info, double* out_cost, void* ws, long workspace_bytes,
                                    void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(model == RANSAC_HOMOGRAPHY || model == RANSAC_FUNDAMENTAL,
               "refine_model: model must be 0 (homography) or 1 (fundamental)");
  ROMA_REQUIRE(M && kpts_a && kpts_b && out_m && out_mask && out_info && out_cost && ws, "refine_model: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= (1 << 16), "refine_model: need 0 <= B <= 65536");
  ROMA_REQUIRE(N >= 0 && (long)B * N < (1l << 31), "refine_model: need 0 <= N, B * N < 2^31");
  ROMA_REQUIRE(thr > 0, "refine_model: threshold must be positive (inf: no truncation)");
  ROMA_REQUIRE(max_steps >= 0 && max_steps <= (1 << 16), "refine_model: need 0 <= max_steps <= 65536");
  ROMA_REQUIRE(ws_bytes >= (size_t)roma_op_refine_model_workspace(B, N), "refine_model: workspace too small (roma_op_refine_model_workspace)");
  if (B == 0) return 0;
  MrState* st;
  model_refine_carve(Workspace256(ws), B, st);
  const float2* ka = reinterpret_cast<const float2*>(kpts_a);
  const float2* kb = reinterpret_cast<const float2*>(kpts_b);
  return model == RANSAC_HOMOGRAPHY
             ? refine_model_run<HomographyFit>(M, ka, kb, counts, valid, B, N, thr, max_steps, out_m, out_mask, out_info, out_cost, st, s)
             : refine_model_run<FundamentalFit>(M, ka, kb, counts, valid, B, N, thr, max_steps, out_m, out_mask, out_info, out_cost, st,
                                                s);
}

}  // namespace roma
