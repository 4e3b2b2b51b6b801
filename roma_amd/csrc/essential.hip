// The essential-matrix (E) model of the device RANSAC (ransac.h) and recoverPose - what the reference's pose benchmarks run on
// sample() output through OpenCV (romatch/utils/utils.py estimate_pose): cv2.findEssentialMat(..., RANSAC) around the
// five-point solver, then cv2.recoverPose.  tools/essential_ref.py restates this file in numpy float64 step by step.
//
// What E adds to the shared pipeline (Essential):
//   normalise   x_n = ((x - cx) / fx, (y - cy) / fy) in f64 (identity without a camera matrix), thr_n = thr / ((fx + fy) / 2).
//               No Hartley normalisation: it would break the essential constraints.
//   hypothesis  16 lanes per hypothesis: the sample's rows normalised in f64 (ransac.h: load_sample), then Nister's five-point
//               solver in f64 (below), up to 10 slots.
//   res_terms   the f32 scoring's terms linear in the model: the epipolar terms (ransac.h: epipolar_terms).
//   inlier      (CountScoring) from them: the Sampson test.  No refinement (REFINE_ITERS = 0: OpenCV has none here).
//   residual2   (MagsacScoring) from them: squared Sampson distance in normalised camera coordinates.
//   wrefit      (MagsacScoring) one IRLS step: the weighted eight-point system over the rows of positive weight, its four smallest
//               eigenvectors as the basis of the solver below, the solution of the smallest score (Essential::wrefit).
//   model_out   E as found or as optimised.  Info rows of ESSENTIAL_INFO (no best_min) and ESSENTIAL_MAGSAC_INFO ints.
//
// The five-point solver (D. Nister, PAMI 2004): null space X, Y, Z, W of the 5 x 9 epipolar system (Gauss-Jordan, then modified
// Gram-Schmidt: an orthonormal basis keeps the elimination below well conditioned), the ten cubic constraints det E = 0 and
// 2 E E^T E - tr(E E^T) E = 0 of E = x X + y Y + z Z + W as a 10 x 20 matrix (one row per lane), Gauss-Jordan on its ten
// leading columns (row swaps and pivot rows by shuffles), the degree-10 polynomial in z as the determinant of Nister's 3 x 3
// polynomial matrix, its real roots by Sturm-sequence bisection with a fixed schedule from Fujiwara's bound (one root per lane,
// ascending: a root's index is its rank) and NEWTON polishing steps, x and y from the two rows of B(z) with the largest cross
// product, then GN_STEPS Gauss-Newton steps of (x, y, z) on the ten cubic constraints themselves (the elimination loses digits
// on some samples; the refinement recovers them), E normalised with its largest-magnitude entry positive.
// recoverPose: ess_decompose_kernel (one-sided Jacobi SVD of E per pair, OpenCV's det fix-up, the four candidates),
// ess_cheirality_kernel (grid (point blocks, pair): triangulation for all four candidates, per-block counts, no atomics),
// ess_pose_kernel (candidate with most good points, ties to the earlier one; R, t, n_good, mask).
// As in the RANSAC pipeline, every flag and count of recoverPose's workspace is written with plain stores by one kernel and read
// by a later launch on the same stream.  Results are bit-identical from run to run and independent of B.
#include "../../include/roma_hip.h"
#include "cheirality.h"
#include "ransac.h"

namespace roma {
namespace {

constexpr int ESSENTIAL_MAX_ROOTS = 10;       // real solutions of one five-point sample (tools/essential_ref.py: MAX_ROOTS)
constexpr int ESSENTIAL_INFO = 5;             // ints per pair in roma_op_essential's out_info
constexpr int ESSENTIAL_MAGSAC_INFO = 7;      // in roma_op_essential_magsac's
constexpr int ESSENTIAL_MAGSAC_MAX_LO = 64;   // largest lo_iters
constexpr int MAXR = ESSENTIAL_MAX_ROOTS;
constexpr int G = 16;                     // lanes per hypothesis in the solver
constexpr int GPB = 256 / G;              // hypotheses per solver workgroup
constexpr int LDS_BASIS = 0, LDS_TAIL = 36, LDS_CHAIN = 96, LDS_PER = 162;  // doubles per hypothesis
constexpr int BISECT = 64;                // bisection steps per root
constexpr int NEWTON = 3;                 // Newton steps on the polynomial after bisection
constexpr double NEWTON_REACH = 1e-3;     // relative length of a Newton step that is still taken
constexpr int GN_STEPS = 3;               // Gauss-Newton steps of (x, y, z) on the cubic constraints
constexpr double GN_REACH = 1e-2;         // relative length of a Gauss-Newton step that is still taken
constexpr double E_PIVOT_EPS = 1e-10;     // |pivot| of the 10 x 20 elimination (unit-norm null basis)
constexpr int SVD_SWEEPS = 20;
constexpr double SVD_TOL = 4 * DBL_EPSILON;

// ------------------------------------------------------------------------------------------------------------ five-point solver
// Nister's column order of the cubic constraints: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ constexpr int mono(int ex, int ey, int ez) {
  switch (ex * 16 + ey * 4 + ez) {
    case 48: return 0;
    case 12: return 1;
    case 36: return 2;
    case 24: return 3;
    case 33: return 4;
    case 32: return 5;
    case 9: return 6;
    case 8: return 7;
    case 21: return 8;
    case 20: return 9;
    case 18: return 10;
    case 17: return 11;
    case 16: return 12;
    case 6: return 13;
    case 5: return 14;
    case 4: return 15;
    case 3: return 16;
    case 2: return 17;
    case 1: return 18;
    default: return 19;
  }
}

// acc += s p q r for three linear polynomials (coefficients of x, y, z, 1)
__device__ __forceinline__ void add_triple(double (&acc)[20], double s, const double* p, const double* q, const double* r) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double pq = s * (p[a] * q[b]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = mono((a == 0) + (b == 0) + (c == 0), (a == 1) + (b == 1) + (c == 1), (a == 2) + (b == 2) + (c == 2));
        acc[k] = acc[k] + pq * r[c];
      }
    }
  }
}

template <int NA, int NB>
__device__ __forceinline__ void pmul(const double (&a)[NA], const double (&b)[NB], double (&c)[NA + NB - 1]) {
#pragma unroll
  for (int k = 0; k < NA + NB - 1; ++k) c[k] = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) c[i + j] = c[i + j] + a[i] * b[j];
}

template <int N>
__device__ __forceinline__ double horner(const double* c, double t) {  // c ascending, N coefficients
  double v = c[N - 1];
#pragma unroll
  for (int i = N - 2; i >= 0; --i) v = v * t + c[i];
  return v;
}

// Nister's 3 x 3 matrix B(z) of <k> = <e> - z <f>, <l> = <g> - z <h>, <m> = <i> - z <j> (rows 4 .. 9 of the reduced
// constraints, columns 10 .. 19): row r = (x coefficient deg 3, y coefficient deg 3, constant deg 4), ascending in z
__device__ __forceinline__ void nister_rows(const double* tail, double (&bx)[3][4], double (&by)[3][4], double (&b1)[3][5]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* e = tail + 20 * r;
    const double* f = e + 10;
    bx[r][0] = e[2]; bx[r][1] = e[1] - f[2]; bx[r][2] = e[0] - f[1]; bx[r][3] = -f[0];
    by[r][0] = e[5]; by[r][1] = e[4] - f[5]; by[r][2] = e[3] - f[4]; by[r][3] = -f[3];
    b1[r][0] = e[9]; b1[r][1] = e[8] - f[9]; b1[r][2] = e[7] - f[8]; b1[r][3] = e[6] - f[7]; b1[r][4] = -f[6];
  }
}

template <int N>
__device__ __forceinline__ void scale_max(double (&p)[N]) {  // divide by the largest magnitude (a positive factor)
  double m = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) m = fmax(m, fabs(p[i]));
  const double inv = 1.0 / m;
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = p[i] * inv;
}

// p_next = -rem(a, b) for deg a = N - 1, deg b = N - 2 (generic degree drop), scaled to unit maximum
template <int N>
__device__ __forceinline__ void sturm_next(const double (&a)[N], const double (&b)[N - 1], double (&r)[N - 2]) {
  const double q1 = a[N - 1] / b[N - 2];
  const double q0 = (a[N - 2] - q1 * b[N - 3]) / b[N - 2];
  r[0] = -(a[0] - q0 * b[0]);
#pragma unroll
  for (int i = 1; i < N - 2; ++i) r[i] = -((a[i] - q1 * b[i - 1]) - q0 * b[i]);
  scale_max(r);
}

template <int N>
__device__ __forceinline__ void store_poly(double* dst, const double (&p)[N], bool w) {
  if (w) {
#pragma unroll
    for (int i = 0; i < N; ++i) dst[i] = p[i];
  }
}

// the chain after a (element 11 - N, N coefficients) and b: element j = 13 - N at offset 11 j - j (j - 1) / 2
template <int N>
__device__ __forceinline__ void sturm_build(const double (&a)[N], const double (&b)[N - 1], double* ch, bool w, double (&lead)[11],
                                            bool& fin) {
  if constexpr (N >= 3) {
    double r[N - 2];
    sturm_next<N>(a, b, r);
    constexpr int j = 13 - N;
    store_poly(ch + 11 * j - j * (j - 1) / 2, r, w);
    lead[j] = r[N - 3];
#pragma unroll
    for (int i = 0; i < N - 2; ++i) fin = fin && isfinite(r[i]);
    sturm_build<N - 1>(b, r, ch, w, lead, fin);
  }
}

// sign changes of the Sturm chain (degrees 10 .. 0, ascending coefficients from offset 0) at t, zeros skipped
__device__ __forceinline__ int sturm_changes(const double* ch, double t) {
  int c = 0;
  double last = 0;
  int off = 0;
#pragma unroll
  for (int k = 0; k <= 10; ++k) {
    const int n = 11 - k;
    double v = ch[off + n - 1];
    for (int i = n - 2; i >= 0; --i) v = v * t + ch[off + i];
    if (v != 0) {
      if (last != 0 && ((v < 0) != (last < 0))) ++c;
      last = v;
    }
    off += n;
  }
  return c;
}

__device__ __forceinline__ void mmt3(const double* a, const double* b, double* c) {  // c = a b^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1]) + a[3 * i + 2] * b[3 * j + 2];
}

// GN_STEPS Gauss-Newton steps of (x, y, z) on the ten cubic constraints of E = x X + y Y + z Z + W themselves (not on the
// eliminated polynomial, whose roots carry the elimination's rounding); a step longer than GN_REACH (1 + max |x, y, z|) or not
// finite is not taken.  3 x 3 normal equations by Cramer's rule.  basis: the group's LDS basis (entry q: x, y, z, 1 coefficients).
__device__ __forceinline__ void refine_xyz(const double* basis, double& x, double& y, double& z) {
  for (int it = 0; it < GN_STEPS; ++it) {
    double E[9], EEt[9], M[9], r[10], J[3][10];
#pragma unroll
    for (int q = 0; q < 9; ++q) E[q] = ((x * basis[4 * q] + y * basis[4 * q + 1]) + z * basis[4 * q + 2]) + basis[4 * q + 3];
    mmt3(E, E, EEt);
    const double tr = (EEt[0] + EEt[4]) + EEt[8];
    mat3(EEt, E, M);
#pragma unroll
    for (int q = 0; q < 9; ++q) r[q] = 2.0 * M[q] - tr * E[q];
    r[9] = det3(E);
    const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                           E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                           E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double D[9], t1[9], t2[9], a1[9], a2[9], a3[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) D[q] = basis[4 * q + k];
      mmt3(D, E, t1);
      mat3(t1, E, a1);
      mmt3(E, D, t2);
      mat3(t2, E, a2);
      mat3(EEt, D, a3);
      double ip = 0, dd = 0;
#pragma unroll
      for (int q = 0; q < 9; ++q) { ip += D[q] * E[q]; dd += cof[q] * D[q]; }
#pragma unroll
      for (int q = 0; q < 9; ++q) J[k][q] = (2.0 * ((a1[q] + a2[q]) + a3[q]) - (2.0 * ip) * E[q]) - tr * D[q];
      J[k][9] = dd;
    }
    double A[9], g[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double gi = 0;
#pragma unroll
      for (int q = 0; q < 10; ++q) gi += J[i][q] * r[q];
      g[i] = gi;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double a = 0;
#pragma unroll
        for (int q = 0; q < 10; ++q) a += J[i][q] * J[j][q];
        A[3 * i + j] = a;
      }
    }
    const double det = det3(A);
    double st[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double Ak[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) Ak[q] = q % 3 == k ? g[q / 3] : A[q];
      st[k] = -det3(Ak) / det;
    }
    const double big = 1.0 + fmax(fmax(fabs(x), fabs(y)), fabs(z));
    const bool take = isfinite(st[0]) && isfinite(st[1]) && isfinite(st[2]) &&
                      fmax(fmax(fabs(st[0]), fabs(st[1])), fabs(st[2])) <= GN_REACH * big;
    x = take ? x + st[0] : x;
    y = take ? y + st[1] : y;
    z = take ? z + st[2] : z;
  }
}

// modified Gram-Schmidt of four vectors in the order X, Y, Z, W; lane 0 of the group stores the basis (entry k of E: the
// coefficients of x, y, z, 1)
__device__ __forceinline__ void store_basis(double (&v)[4][9], double* sm, int gl) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#pragma unroll
    for (int g = 0; g < f; ++g) {
      double d = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) d += v[f][k] * v[g][k];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[f][k] = v[f][k] - d * v[g][k];
    }
    double s = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) s += v[f][k] * v[f][k];
    const double inv = 1.0 / sqrt(s);
#pragma unroll
    for (int k = 0; k < 9; ++k) v[f][k] = v[f][k] * inv;
    if (gl == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) sm[LDS_BASIS + 4 * k + f] = v[f][k];
    }
  }
}

__device__ __forceinline__ void solve_e_basis(bool act, double* sm, int gl, double (&e)[9], int& rank, int& nsol);

// One hypothesis on the G lanes of a group (gl = lane in the group); every lane of the workgroup must call it (barriers).
// Returns this lane's model in e (valid: a real root whose E is finite), its rank among the group's valid models and their
// number.  sm: the group's LDS_PER doubles.
__device__ __forceinline__ void solve_e_group(const double (&xa)[5], const double (&ya)[5], const double (&xb)[5], const double (&yb)[5], bool act,
                              double* sm, int gl, double (&e)[9], int& rank, int& nsol) {
  // null space of the 5 x 9 system x1^T E x0 = 0 (every lane, registers); basis X, Y, Z, W = free columns 5 .. 8, unit norm
  {
    double a[5][9];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double x = xa[k], y = ya[k], u = xb[k], v = yb[k];
      a[k][0] = u * x; a[k][1] = u * y; a[k][2] = u; a[k][3] = v * x; a[k][4] = v * y; a[k][5] = v;
      a[k][6] = x; a[k][7] = y; a[k][8] = 1;
    }
    act = gauss_jordan(a) && act;
    double v[4][9];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int k = 0; k < 5; ++k) v[f][k] = -a[k][5 + f];
#pragma unroll
      for (int k = 5; k < 9; ++k) v[f][k] = k == 5 + f ? 1.0 : 0.0;
    }
    store_basis(v, sm, gl);
  }
  solve_e_basis(act, sm, gl, e, rank, nsol);
}

// The solver from the group's basis X, Y, Z, W in LDS on (store_basis; the barrier that publishes it is the first thing here):
// the real E = x X + y Y + z Z + W that satisfy the cubic constraints.  A five-point sample's null space (solve_e_group), or
// the least-squares null space of more rows (Essential::wrefit) - Nister's form for more than five points.
__device__ __forceinline__ void solve_e_basis(bool act, double* sm, int gl, double (&e)[9], int& rank, int& nsol) {
  __syncthreads();
  // row gl of the 10 x 20 constraint matrix: 2 (E E^T E)_ij - tr(E E^T) E_ij for gl = 3 i + j < 9, det E for gl = 9
  double acc[20];
#pragma unroll
  for (int k = 0; k < 20; ++k) acc[k] = 0;
  const double* P = sm + LDS_BASIS;
  if (gl < 9) {
    const int i = gl / 3, j = gl % 3;
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) {
        add_triple(acc, 2.0, P + 4 * (3 * i + l), P + 4 * (3 * k + l), P + 4 * (3 * k + j));
        add_triple(acc, -1.0, P + 4 * (3 * k + l), P + 4 * (3 * k + l), P + 4 * (3 * i + j));
      }
  } else if (gl == 9) {
    constexpr int perm[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};
    for (int q = 0; q < 6; ++q)
      add_triple(acc, q < 3 ? 1.0 : -1.0, P + 4 * perm[q][0], P + 4 * (3 + perm[q][1]), P + 4 * (6 + perm[q][2]));
  }
  // Gauss-Jordan on columns 0 .. 9 with partial pivoting (first maximum); lane r holds row r
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    double v = gl >= k && gl < 10 ? fabs(acc[k]) : -1.0;
    int p = gl;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      const double ov = __shfl_xor(v, off, G);
      const int op = __shfl_xor(p, off, G);
      if (ov > v || (ov == v && op < p)) { v = ov; p = op; }
    }
    act = act && v > E_PIVOT_EPS;
    const int src = gl == k ? p : gl == p ? k : gl;
#pragma unroll
    for (int c = 0; c < 20; ++c) acc[c] = __shfl(acc[c], src, G);
    const double inv = 1.0 / __shfl(acc[k], k, G);
    if (gl == k) {
#pragma unroll
      for (int c = 0; c < 20; ++c) acc[c] = acc[c] * inv;
    }
    const double f = acc[k];
#pragma unroll
    for (int c = 0; c < 20; ++c) {
      const double rk = __shfl(acc[c], k, G);
      if (gl != k) acc[c] = acc[c] - f * rk;
    }
  }
  if (gl >= 4 && gl < 10) {
#pragma unroll
    for (int c = 0; c < 10; ++c) sm[LDS_TAIL + 10 * (gl - 4) + c] = acc[10 + c];
  }
  __syncthreads();
  // degree-10 polynomial det B(z) and its Sturm chain (every lane the same values; lane 0 stores the chain)
  double bx[3][4], by[3][4], b1[3][5];
  nister_rows(sm + LDS_TAIL, bx, by, b1);
  double lead[11];
  bool fin = true;
  double bound;
  {
    double u0[8], u1[8], v0[8], v1[8], w0[7], w1[7];
    pmul(by[1], b1[2], u0);
    pmul(b1[1], by[2], u1);
    pmul(bx[1], b1[2], v0);
    pmul(b1[1], bx[2], v1);
    pmul(bx[1], by[2], w0);
    pmul(by[1], bx[2], w1);
#pragma unroll
    for (int i = 0; i < 8; ++i) { u0[i] = u0[i] - u1[i]; v0[i] = v0[i] - v1[i]; }
#pragma unroll
    for (int i = 0; i < 7; ++i) w0[i] = w0[i] - w1[i];
    double p0[11], q0[11], q1[11], p1[10];
    pmul(bx[0], u0, p0);
    pmul(by[0], v0, q0);
    pmul(b1[0], w0, q1);
#pragma unroll
    for (int i = 0; i < 11; ++i) p0[i] = (p0[i] - q0[i]) + q1[i];
    scale_max(p0);
#pragma unroll
    for (int i = 0; i < 10; ++i) p1[i] = (i + 1) * p0[i + 1];
    scale_max(p1);
    double* ch = sm + LDS_CHAIN;
    store_poly(ch, p0, gl == 0);
    store_poly(ch + 11, p1, gl == 0);
    lead[0] = p0[10];
    lead[1] = p1[9];
#pragma unroll
    for (int i = 0; i < 11; ++i) fin = fin && isfinite(p0[i]);
#pragma unroll
    for (int i = 0; i < 10; ++i) fin = fin && isfinite(p1[i]);
    sturm_build<11>(p0, p1, ch, gl == 0, lead, fin);
    bound = 0;
#pragma unroll
    for (int i = 1; i <= 10; ++i) bound = fmax(bound, pow(fabs(p0[10 - i] / p0[10]), 1.0 / i));
    bound = 2.0 * bound;  // Fujiwara's bound of the roots: 2 max_i |a_{10-i} / a_10|^(1/i)
  }
  // sign changes at -inf and +inf from the leading coefficients (degree of element j: 10 - j)
  int vneg = 0, vpos = 0;
  {
    double ln = 0, lp = 0;
#pragma unroll
    for (int j = 0; j <= 10; ++j) {
      fin = fin && lead[j] != 0;
      const double a = lead[j], an = (10 - j) % 2 ? -a : a;
      if (lp != 0 && ((a < 0) != (lp < 0))) ++vpos;
      if (ln != 0 && ((an < 0) != (ln < 0))) ++vneg;
      lp = a;
      ln = an;
    }
  }
  fin = fin && isfinite(bound);
  const int nroots = fin && act ? min(max(vneg - vpos, 0), MAXR) : 0;
  __syncthreads();
  // root gl (ascending) by bisection on the number of roots in (-inf, t]
  double lo = -bound, hi = bound;
  for (int it = 0; it < BISECT; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool up = vneg - sturm_changes(sm + LDS_CHAIN, mid) >= gl + 1;
    lo = up ? lo : mid;
    hi = up ? mid : hi;
  }
  double z = 0.5 * (lo + hi);
  {  // Newton polish on p0; a step longer than NEWTON_REACH (1 + |z|) is not taken
    const double* p0 = sm + LDS_CHAIN;
    for (int it = 0; it < NEWTON; ++it) {
      double v = p0[10], d = 10 * p0[10];
#pragma unroll
      for (int i = 9; i >= 0; --i) {
        v = v * z + p0[i];
        if (i > 0) d = d * z + i * p0[i];
      }
      const double z1 = z - v / d;
      z = isfinite(z1) && fabs(z1 - z) <= NEWTON_REACH * (1.0 + fabs(z)) ? z1 : z;
    }
  }
  // x, y from the null vector of B(z): the cross product of two rows with the largest |w| (first on ties)
  double rx[3], ry[3], r1[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) { rx[r] = horner<4>(bx[r], z); ry[r] = horner<4>(by[r], z); r1[r] = horner<5>(b1[r], z); }
  double c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
  for (int pr = 0; pr < 3; ++pr) {
    const int a = pr == 2 ? 1 : 0, b = pr == 0 ? 1 : 2;
    const double d0 = ry[a] * r1[b] - r1[a] * ry[b], d1 = r1[a] * rx[b] - rx[a] * r1[b], d2 = rx[a] * ry[b] - ry[a] * rx[b];
    if (fabs(d2) > fabs(c2)) { c0 = d0; c1 = d1; c2 = d2; }
  }
  double x = c0 / c2, y = c1 / c2;
  refine_xyz(sm + LDS_BASIS, x, y, z);
  double s = 0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const double* b = sm + LDS_BASIS + 4 * q;
    e[q] = ((x * b[0] + y * b[1]) + z * b[2]) + b[3];
    s += e[q] * e[q];
  }
  const double inv = 1.0 / sqrt(s);
  int big = 0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    e[q] = e[q] * inv;
    if (fabs(e[q]) > fabs(e[big])) big = q;
  }
  bool valid = gl < nroots;
  double sg = 1.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    valid = valid && isfinite(e[q]);
    if (q == big && e[q] < 0) sg = -1.0;
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) e[q] = e[q] * sg;
  const unsigned long long bal = __ballot(valid);
  const unsigned gm = (unsigned)(bal >> (threadIdx.x & 63 & ~(G - 1))) & ((1u << G) - 1);
  rank = valid ? __popc(gm & ((1u << gl) - 1)) : -1;
  nsol = __popc(gm);
  __syncthreads();  // the group's LDS is reused by the caller's next hypothesis
}

// ------------------------------------------------------------------------------------------------------------ 3 x 3 SVD
// A = U S V^T by one-sided Jacobi on the columns of A (A V = U S).  a[j]: column j of A on entry, of U S on return; v[j]: column
// j of V (identity on entry); sg: the singular values, descending (columns of a and v sorted with them).  run = false skips
// the sweeps (a matrix that is not finite).
__device__ __forceinline__ void jacobi_svd3(double (&a)[3][3], double (&v)[3][3], double (&sg)[3], bool run) {
  for (int sweep = 0; sweep < SVD_SWEEPS && run; ++sweep) {
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
      if (fabs(ga) > SVD_TOL * sqrt(al * be)) {
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
#pragma unroll
  for (int j = 0; j < 3; ++j) sg[j] = sqrt(a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2]);
  // sort descending (columns of A and V together)
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
}

// ------------------------------------------------------------------------------------------------------------ model policy
struct Essential : Terms<Essential> {
  struct Norm {
    double fx, fy, cx, cy;  // x_n = (x - c) / f
    __device__ void apply(float2 a, float2 q, double& xa, double& ya, double& xb, double& yb) const {
      xa = (a.x - cx) / fx; ya = (a.y - cy) / fy;
      xb = (q.x - cx) / fx; yb = (q.y - cy) / fy;
    }
  };
  using In = PairIn;
  using Rows = PairRows;
  using Out = double*;  // [B, 9]
  static constexpr int S = 5, SLOTS = MAXR, NM = 9, MIN_INLIERS = 1, HYP_THREADS = 256, HYP_LANES = G, REFINE_ITERS = 0;
  static constexpr int INFO = ESSENTIAL_INFO;
  static constexpr int MAG_INFO = ESSENTIAL_MAGSAC_INFO, NT = 5, REFIT_MIN = 8;  // MAGSAC++: info, residual terms, rows of a step
  static constexpr bool SCORE_EVERY_SLOT = false;  // 10 slots, a few of them used: score only those

  // every thread of the workgroup: the pair's camera; pts written for every row; one threshold (t2a == t2b)
  __device__ static bool normalise(PairIn in, int n, const double* K, float thr, double* sh, PairRows rows, Norm& nm, float& t2a,
                                   float& t2b) {
    const float2 *A = in.a, *Bp = in.b;
    float4* pts = rows.p;
    const int t = threadIdx.x;
    double fx = 1, fy = 1, cx = 0, cy = 0;
    if (K) {
      fx = K[0]; cx = K[2]; fy = K[4]; cy = K[5];
    }
    const double thr_n = (double)thr / ((fx + fy) * 0.5);
    double cnt = 0;
    for (int i = t; i < n; i += 256) {
      const float2 a = A[i], q = Bp[i];
      const bool f = finite_row(a.x, a.y, q.x, q.y);
      cnt += f ? 1 : 0;
      float4 o = make_float4(NAN, NAN, NAN, NAN);
      if (f) o = make_float4((float)((a.x - cx) / fx), (float)((a.y - cy) / fy), (float)((q.x - cx) / fx), (float)((q.y - cy) / fy));
      pts[i] = o;
    }
    cnt = block_sum(cnt, sh);
    nm.fx = fx; nm.fy = fy; nm.cx = cx; nm.cy = cy;
    t2a = t2b = (float)(thr_n * thr_n);
    return cnt >= S && fx != 0 && fy != 0 && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) && thr_n > 0 &&
           isfinite(thr_n);
  }

  // the G lanes of a group: the hypothesis' valid models in slots 0 .. nsol - 1
  __device__ static void hypothesis(PairIn in, const int (&idx)[S], bool act, const Norm& nrm, int g, int gl, const Slots& sl) {
    __shared__ double sm[GPB * LDS_PER];
    double xa[S], ya[S], xb[S], yb[S];
    act = load_sample(in, idx, act, nrm, xa, ya, xb, yb);
    double e[9];
    int rank, nsol;
    solve_e_group(xa, ya, xb, yb, act, sm + (threadIdx.x / G) * LDS_PER, gl, e, rank, nsol);
    if (rank >= 0) store_model(e, (long)g * MAXR + rank, sl);
    if (gl == 0) sl.n[g] = nsol;
  }

  // the f32 scoring on the epipolar terms (d, l_x, l_y, k_x, k_y) of p = (x0, y0, x1, y1) normalised.  Sampson test in
  // multiplication form: (x1^T E x0)^2 < thr^2 (|E x0|_{1,2}^2 + |E^T x1|_{1,2}^2); MAGSAC++: the squared Sampson distance
  // d^2 / ((l_x^2 + l_y^2) + (k_x^2 + k_y^2)) - the same quantities, so r^2 < thr^2 is that test up to the rounding of the division
  __device__ static void res_terms(const float* m, float4 p, float (&t)[NT]) { epipolar_terms(m, p, t); }
  __device__ static bool inlier_from(const float (&t)[NT], float t2, float) {
    return t[0] * t[0] < t2 * (fmaf(t[1], t[1], t[2] * t[2]) + fmaf(t[3], t[3], t[4] * t[4]));
  }
  __device__ static float r2_from(const float (&t)[NT], float, float) {
    return t[0] * t[0] / (fmaf(t[1], t[1], t[2] * t[2]) + fmaf(t[3], t[3], t[4] * t[4]));
  }

  // ---- MAGSAC++ (MagsacScoring): residuals in normalised camera coordinates, so no scales and tau = thr_n of normalise
  __device__ static void res_scales(const Norm&, float& sa2, float& sb2) { sa2 = sb2 = 1.f; }
  __device__ static double mag_thr2(const Norm& nm, float thr) {
    const double thr_n = (double)thr / ((nm.fx + nm.fy) * 0.5);
    return thr_n * thr_n;
  }

  // One IRLS step of the local optimisation, every thread of the 256 (ransac_refit_kernel):
  //   1. over the rows of positive MAGSAC++ weight under the current model (at least REFIT_MIN, else LO stops): Hartley
  //      normalisation of both images (hartley_moments), then the weighted eight-point normal equations sum w_i a_i a_i^T
  //      (normal_equations: what Hartley<>::fit runs);
  //   2. wave 0: their eigenvectors by one-sided Jacobi; those of the four smallest eigenvalues, de-normalised (Tb^T F_n Ta),
  //      span the least-squares null space;
  //   3. the five-point solver on that basis (solve_e_basis; W the smallest eigenvector): the E of the span that satisfy the
  //      cubic constraints.  The smallest eigenvector alone, projected onto the essential manifold, is the eight-point
  //      algorithm - on scenes close to a plane it follows the noise (tools/essential_magsac_ref.py);
  //   4. wave 0: the sum of rho of each solution (magsac_sums), the smallest one (lowest slot on ties) projected onto the
  //      essential manifold (singular values ((s1 + s2) / 2, (s1 + s2) / 2, 0): exact where the solver's root was not), unit
  //      norm, largest-magnitude entry positive -> P.cand.
  // Every group of the workgroup runs step 3 on the same basis (the solver's barriers need every thread); group 0's is used.
  __device__ static void wrefit(const float2* A, const float2* Bp, const float4* pts, PairState<Essential>& P, const MagState& S) {
    __shared__ double sm[GPB * LDS_PER];
    __shared__ double sh[256];
    __shared__ double Mx[9][9];
    __shared__ double ev[4][9];
    __shared__ double cd[MAXR][9];
    __shared__ alignas(16) float cf[MAXR * 12];
    __shared__ int ncand;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = P.n;
    const bool run = !P.stop && P.best_h >= 0;
    float curf[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) curf[k] = P.curf[k];
    const double fx = P.nrm.fx, fy = P.nrm.fy, cx = P.nrm.cx, cy = P.nrm.cy;
    const float vs = S.vs;
    __syncthreads();  // the pair's flags are read; thread 0 may rewrite them from here on
    if (!run) {
      if (t == 0) { P.stop = 1; P.cand_ok = 0; }
      return;
    }
    // 1. Hartley normalisation over the rows of positive weight (NaN rows have none)
    const auto weight = [&](int i, float& w) {
      magsac_rho(residual2(curf, pts[i], 1.f, 1.f) * vs, w);
      return w > 0.f;
    };
    const HartleyMoments hm = hartley_moments(n, [&](int i, double& ax, double& ay, double& bx, double& by) {
      float w;
      if (!weight(i, w)) return false;
      const float2 a = A[i], q = Bp[i];
      ax = (a.x - cx) / fx; ay = (a.y - cy) / fy; bx = (q.x - cx) / fx; by = (q.y - cy) / fy;
      return true;
    }, sh);
    if (!hm.ok(REFIT_MIN)) {  // uniform: block_sum's value
      if (t == 0) { P.stop = 1; P.cand_ok = 0; }
      return;
    }
    const double cax = hm.cax, cay = hm.cay, cbx = hm.cbx, cby = hm.cby, sa = hm.sa, sb = hm.sb;
    if (t >= 45 && t < 45 + 36)
      ev[(t - 45) / 9][(t - 45) % 9] = 0.0;  // a system that is not finite ranks no eigenvector: a zero basis has no solution
    normal_equations<true, false>(n, [&](int i, double& wt) {
      float w;
      const bool pos = weight(i, w);
      wt = w;
      return pos;
    }, [&](int i, double (&r1)[9], double (&)[9]) {
      const float2 a = A[i], q = Bp[i];
      const double x = ((a.x - cx) / fx - cax) * sa, y = ((a.y - cy) / fy - cay) * sa;
      const double u = ((q.x - cx) / fx - cbx) * sb, v = ((q.y - cy) / fy - cby) * sb;
      const double e1[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1};
#pragma unroll
      for (int k = 0; k < 9; ++k) r1[k] = e1[k];
    }, Mx);
    // 2. the eigenvectors of the four smallest eigenvalues (ties: the lower lane first), de-normalised: ev[0 .. 3] = X, Y, Z, W
    if (wave == 0) {
      double col[9], vv[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        col[k] = lane < 9 ? Mx[k][lane] : 0.0;
        vv[k] = lane == k ? 1.0 : 0.0;
      }
      jacobi_sweeps<9, 10>(col, vv, lane);
      const double lam = jacobi_eigenvalue<9>(col, lane);
      int rk = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const double lj = __shfl(lam, j);
        rk += lj < lam || (lj == lam && j < lane) ? 1 : 0;
      }
      if (lane < 9 && rk < 4) {
        const double ta[9] = {sa, 0, -sa * cax, 0, sa, -sa * cay, 0, 0, 1};
        const double tbt[9] = {sb, 0, 0, 0, sb, 0, -sb * cbx, -sb * cby, 1};
        double tmp[9], f[9];
        mat3(tbt, vv, tmp);
        mat3(tmp, ta, f);
#pragma unroll
        for (int k = 0; k < 9; ++k) ev[3 - rk][k] = f[k];
      }
    }
    __syncthreads();
    // 3. the solver on the basis
    double* smg = sm + (t / G) * LDS_PER;
    const int gl = t % G;
    {
      double v[4][9];
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int k = 0; k < 9; ++k) v[f][k] = ev[f][k];
      store_basis(v, smg, gl);
    }
    double e[9];
    int rank, nsol;
    solve_e_basis(true, smg, gl, e, rank, nsol);
    if (t < G) {
      if (rank >= 0) {
        float mf[12];
        to_f32(e, mf);
#pragma unroll
        for (int k = 0; k < 9; ++k) cd[rank][k] = e[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) cf[12 * rank + k] = mf[k];
      }
      if (t == 0) ncand = nsol;
    }
    __syncthreads();
    // 4. the solution of the smallest score
    if (wave != 0) return;
    const int nm = ncand;
    if (nm == 0) {
      if (lane == 0) { P.stop = 1; P.cand_ok = 0; }
      return;
    }
    float sc[MAXR];
    int ct[MAXR];
    magsac_sums<Essential, MAXR>(cf, nm, pts, n, S, lane, sc, ct);
    int bs = 0;
    float bv = sc[0];
#pragma unroll
    for (int r = 1; r < MAXR; ++r)
      if (r < nm && sc[r] < bv) { bv = sc[r]; bs = r; }
    if (lane != 0) return;
    double a[3][3], v[3][3], sg[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        a[j][i] = cd[bs][3 * i + j];
        v[j][i] = i == j ? 1.0 : 0.0;
      }
    jacobi_svd3(a, v, sg, true);
    const double sm2 = 0.5 * (sg[0] + sg[1]);
    double m[9], fro = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        m[3 * i + k] = sm2 * ((a[0][i] / sg[0]) * v[0][k] + (a[1][i] / sg[1]) * v[1][k]);
        fro += m[3 * i + k] * m[3 * i + k];
      }
    const double inv = 1.0 / sqrt(fro);
    int big = 0;
    bool ok = sg[1] > 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      m[k] = m[k] * inv;
      ok = ok && isfinite(m[k]);
      if (fabs(m[k]) > fabs(m[big])) big = k;
    }
    double sgn = 1.0;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (k == big && m[k] < 0) sgn = -1.0;
    P.cand_ok = ok ? 1 : 0;
    if (ok) {
      for (int k = 0; k < 9; ++k) P.cand[k] = m[k] * sgn;
      to_f32(P.cand, P.candf);
    } else {
      P.stop = 1;
    }
  }

  // E as found or as optimised
  __device__ static void model_out(const PairState<Essential>& P, bool good, double* out, int b) {
    for (int k = 0; k < 9; ++k) out[(long)b * 9 + k] = good ? P.cur[k] : 0.0;
  }
};

// the solver alone on caller samples; grid ceil(S / GPB)
__global__ __launch_bounds__(256) void ess_minimal_kernel(const double* __restrict__ x0, const double* __restrict__ x1, int S,
                                                          double* __restrict__ out_e, int* __restrict__ out_n) {
  __shared__ double sm[GPB * LDS_PER];
  const int grp = threadIdx.x / G, gl = threadIdx.x % G;
  const int s = blockIdx.x * GPB + grp;
  const bool act = s < S;
  double xa[5], ya[5], xb[5], yb[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const long o = ((long)(act ? s : 0) * 5 + k) * 2;
    xa[k] = x0[o]; ya[k] = x0[o + 1]; xb[k] = x1[o]; yb[k] = x1[o + 1];
  }
  double e[9];
  int rank, nsol;
  solve_e_group(xa, ya, xb, yb, act, sm + grp * LDS_PER, gl, e, rank, nsol);
  if (!act) return;
  if (rank >= 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) out_e[((long)s * MAXR + rank) * 9 + k] = e[k];
  }
  if (gl >= nsol && gl < MAXR) {
#pragma unroll
    for (int k = 0; k < 9; ++k) out_e[((long)s * MAXR + gl) * 9 + k] = 0.0;
  }
  if (gl == 0) out_n[s] = nsol;
}

// ------------------------------------------------------------------------------------------------------------ recoverPose
struct PoseState {
  double cand[4][12];           // (R row-major, t) of the four candidates: (R1, t), (R2, t), (R1, -t), (R2, -t)
  double fx, fy, cx, cy;
  int n, valid;
};

// one thread per pair: E = U S V^T by one-sided Jacobi on the columns of E (A V = U S), singular values descending,
// u3 = u1 x u2 (v3 signed to match where s3 > 0), OpenCV's fix-up (det(U), det(V) > 0), W = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]],
// R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]
__global__ __launch_bounds__(64) void ess_decompose_kernel(const double* __restrict__ E, const int* __restrict__ counts,
                                                           const double* __restrict__ K, int B, int N, PoseState* __restrict__ st) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double a[3][3], v[3][3];  // a[j] = column j
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      a[j][i] = E[(long)b * 9 + 3 * i + j];
      fin = fin && isfinite(a[j][i]);
      v[j][i] = i == j ? 1.0 : 0.0;
    }
  double sg[3];
  jacobi_svd3(a, v, sg, fin);
  double U[9], Vt[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    U[3 * k] = a[0][k] / sg[0];
    U[3 * k + 1] = a[1][k] / sg[1];
  }
  U[2] = U[3] * U[7] - U[6] * U[4];
  U[5] = U[6] * U[1] - U[0] * U[7];
  U[8] = U[0] * U[4] - U[3] * U[1];
  const double d3 = a[2][0] * U[2] + a[2][1] * U[5] + a[2][2] * U[8];
  const double s3 = d3 < 0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Vt[k] = v[0][k];
    Vt[3 + k] = v[1][k];
    Vt[6 + k] = s3 * v[2][k];
  }
  const double dv = Vt[0] * (Vt[4] * Vt[8] - Vt[5] * Vt[7]) - Vt[1] * (Vt[3] * Vt[8] - Vt[5] * Vt[6]) +
                    Vt[2] * (Vt[3] * Vt[7] - Vt[4] * Vt[6]);
  if (dv < 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Vt[k] = -Vt[k];
  }
  const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, Wt[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
  double tmp[9], R1[9], R2[9];
  mat3(U, W, tmp);
  mat3(tmp, Vt, R1);
  mat3(U, Wt, tmp);
  mat3(tmp, Vt, R2);
  bool ok = fin && sg[1] > 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && isfinite(R1[k]) && isfinite(R2[k]) && isfinite(U[k]);
  PoseState& P = st[b];
  for (int c = 0; c < 4; ++c) {
    const double* Rc = c % 2 == 0 ? R1 : R2;
    const double ts = c < 2 ? 1.0 : -1.0;
    for (int k = 0; k < 9; ++k) P.cand[c][k] = Rc[k];
    for (int k = 0; k < 3; ++k) P.cand[c][9 + k] = ts * U[3 * k + 2];
  }
  double fx = 1, fy = 1, cx = 0, cy = 0;
  if (K) {
    const double* k = K + (long)b * 9;
    fx = k[0]; cx = k[2]; fy = k[4]; cy = k[5];
  }
  P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy;
  P.n = counts ? min(max(counts[b], 0), N) : N;
  P.valid = ok && fx != 0 && fy != 0 && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) ? 1 : 0;
}

// grid (ceil(N / 256), B): good flags of the four candidates per point, per-block counts
__global__ __launch_bounds__(256) void ess_cheirality_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb,
                                                             const unsigned char* __restrict__ mask, int N, double dist,
                                                             const PoseState* __restrict__ st, unsigned char* __restrict__ flags,
                                                             int* __restrict__ partial) {
  __shared__ int sh[4][4];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PoseState& P = st[b];
  int bits = 0;
  if (P.valid && i < P.n && (!mask || mask[(long)b * N + i])) {
    const float2 a = ka[(long)b * N + i], q = kb[(long)b * N + i];
    if (finite_row(a.x, a.y, q.x, q.y)) {
      const double x = (a.x - P.cx) / P.fx, y = (a.y - P.cy) / P.fy, u = (q.x - P.cx) / P.fx, v = (q.y - P.cy) / P.fy;
#pragma unroll
      for (int c = 0; c < 4; ++c) bits |= cheiral(P.cand[c], x, y, u, v, dist) ? 1 << c : 0;
    }
  }
  if (i < N) flags[(long)b * N + i] = (unsigned char)bits;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int n = __popcll(__ballot((bits >> c) & 1));
    if (lane == 0) sh[wave][c] = n;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    partial[((long)b * gridDim.x + blockIdx.x) * 4 + c] = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
  }
}

// one workgroup per pair: candidate with the most good points (ties: the earlier one), R, t, n_good, mask_good
__global__ __launch_bounds__(256) void ess_pose_kernel(int N, int nblk, const PoseState* __restrict__ st,
                                                       const unsigned char* __restrict__ flags, const int* __restrict__ partial,
                                                       int* __restrict__ out_n, double* __restrict__ out_r, double* __restrict__ out_t,
                                                       unsigned char* __restrict__ out_mask) {
  __shared__ int best;
  const int b = blockIdx.x, t = threadIdx.x;
  const PoseState& P = st[b];
  if (t == 0) {
    int cnt[4] = {0, 0, 0, 0};
    for (int k = 0; k < nblk; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) cnt[c] += partial[((long)b * nblk + k) * 4 + c];
    int bc = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c)
      if (cnt[c] > cnt[bc]) bc = c;
    best = bc;
    const bool ok = P.valid;
    out_n[b] = ok ? cnt[bc] : 0;
    for (int k = 0; k < 9; ++k) out_r[(long)b * 9 + k] = ok ? P.cand[bc][k] : 0.0;
    for (int k = 0; k < 3; ++k) out_t[(long)b * 3 + k] = ok ? P.cand[bc][9 + k] : 0.0;
  }
  __syncthreads();
  const int c = best;
  for (int i = t; i < N; i += 256) out_mask[(long)b * N + i] = (unsigned char)((flags[(long)b * N + i] >> c) & 1);
}

struct PoseCarve {
  PoseState* st;
  unsigned char* flags;
  int* partial;
  size_t bytes;
};

PoseCarve pose_carve(Workspace256 ws, int B, int N) {
  PoseCarve c;
  const size_t nblk = (N + 255) / 256;
  c.st = ws.take<PoseState>(B);
  c.flags = ws.take<unsigned char>((size_t)B * N);
  c.partial = ws.take<int>(4 * nblk * B);
  c.bytes = ws.bytes();
  return c;
}

static_assert(MagsacScoring::MAX_STEPS == ESSENTIAL_MAGSAC_MAX_LO);

// the check and launch behind roma_op_essential and roma_op_essential_magsac: `opt` is `lo_iters`, out_score NULL without scores
template <class Sc>
int e_launch(const char* op, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
             const double* K, int B, int N, float threshold, double prob, int max_iters, int opt, double* out_e,
             unsigned char* out_mask, unsigned char* out_ok, int* out_info, double* out_score, void* ws, size_t ws_bytes,
             hipStream_t s) {
  if (check_args<Sc>(op, "prob", kpts_a && kpts_b && seeds && out_e && out_mask && out_ok && out_info && (out_score || !Sc::SCORES) && ws,
                     B, N, threshold, prob, max_iters, opt, ws_bytes, workspace_bytes<Essential, Sc>(B, N)))
    return -1;
  return ransac_run<Essential, Sc>({reinterpret_cast<const float2*>(kpts_a), reinterpret_cast<const float2*>(kpts_b)}, counts, seeds, K, B, N, threshold, prob, max_iters, opt, out_e, out_mask, out_ok,
                                   out_info, out_score, ws, s);
}

}  // namespace

extern "C" long roma_op_essential_workspace(int B, int N) { return (long)workspace_bytes<Essential, CountScoring>(B, N); }

extern "C" int roma_op_essential(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                                 const double* K, int B, int N, float threshold, double prob, int max_iters, double* out_e,
                                 unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* ws, long ws_bytes, void* stream) {
  return e_launch<CountScoring>("essential", kpts_a, kpts_b, counts, seeds, K, B, N, threshold, prob, max_iters, 0, out_e, out_mask,
                                out_ok, out_info, nullptr, ws, workspace_size(ws_bytes), static_cast<hipStream_t>(stream));
}

extern "C" long roma_op_essential_magsac_workspace(int B, int N) { return (long)workspace_bytes<Essential, MagsacScoring>(B, N); }

extern "C" int roma_op_essential_magsac(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                                        const double* K, int B, int N, float threshold, double prob, int max_iters, int lo_iters,
                                        double* out_e, unsigned char* out_mask, unsigned char* out_ok, int* out_info, double* out_score,
                                        void* ws, long ws_bytes, void* stream) {
  return e_launch<MagsacScoring>("essential_magsac", kpts_a, kpts_b, counts, seeds, K, B, N, threshold, prob, max_iters, lo_iters,
                                 out_e, out_mask, out_ok, out_info, out_score, ws, workspace_size(ws_bytes),
                                 static_cast<hipStream_t>(stream));
}

extern "C" int roma_op_essential_minimal(const double* x0, const double* x1, int S, double* out_e, int* out_n, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(x0 && x1 && out_e && out_n, "essential_minimal: null pointer");
  ROMA_REQUIRE(S > 0 && S <= (1 << 24), "essential_minimal: need 0 < S <= 2^24");
  hipLaunchKernelGGL(ess_minimal_kernel, dim3((S + GPB - 1) / GPB), dim3(256), 0, s, x0, x1, S, out_e, out_n);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" long roma_op_recover_pose_workspace(int B, int N) {
  return B > 0 && N > 0 ? (long)pose_carve(Workspace256(), B, N).bytes : 0;
}

extern "C" int roma_op_recover_pose(const double* E, const float* kpts_a, const float* kpts_b, const unsigned char* mask,
                                    const int* counts, const double* K, int B, int N, double distance_thresh, int* out_n, double* out_r,
                                    double* out_t, unsigned char* out_mask, void* ws, long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(E && kpts_a && kpts_b && out_n && out_r && out_t && out_mask && ws, "recover_pose: null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16), "recover_pose: need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(distance_thresh > 0, "recover_pose: distance_thresh must be positive");
  ROMA_REQUIRE(ws_bytes >= (size_t)roma_op_recover_pose_workspace(B, N), "recover_pose: workspace too small (roma_op_recover_pose_workspace)");
  const PoseCarve c = pose_carve(Workspace256(ws), B, N);
  const int nblk = (N + 255) / 256;
  hipLaunchKernelGGL(ess_decompose_kernel, dim3((B + 63) / 64), dim3(64), 0, s, E, counts, K, B, N, c.st);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(ess_cheirality_kernel, dim3(nblk, B), dim3(256), 0, s, reinterpret_cast<const float2*>(kpts_a),
                     reinterpret_cast<const float2*>(kpts_b), mask, N, distance_thresh, c.st, c.flags, c.partial);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(ess_pose_kernel, dim3(B), dim3(256), 0, s, N, nblk, c.st, c.flags, c.partial, out_n, out_r, out_t, out_mask);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
