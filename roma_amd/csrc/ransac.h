// Batched robust estimation on the device: one pipeline for every model and every scoring, templated on a model policy M
// (geometry.hip: homography and fundamental matrix; essential.hip: essential matrix; absolute_pose.hip: camera pose from 3-D
// points) and a scoring policy Sc (below: CountScoring - RANSAC's inlier count; MagsacScoring - MAGSAC++).
// tools/geometry_ref.py restates it in numpy float64 (round_loop) and is, with the models' and scorings' own restatements,
// the oracle of the GPU tests.
//
// What a model supplies:
//   S, SLOTS, NM          rows of a minimal sample, models it can yield, doubles per model (9: a 3 x 3 matrix; 12: R and t)
//   HYP_THREADS, HYP_LANES  workgroup size of ransac_hyp_kernel and lanes per hypothesis
//   MIN_INLIERS           inliers below which a pair has no model (mask, ok)
//   REFINE_ITERS, INFO, SCORE_EVERY_SLOT   least-squares refits under CountScoring (0: none; then refit is not needed), ints of
//                         its info row (INFO_CORE, or one more: best_min), whether unused slots are scored as well (they hold zeros)
//   In, Out               the caller's arrays, as passed to ransac_run: In has at(row) - the same arrays from that row on (the
//                         two-view models: PairIn); Out is what model_out writes (the two-view models: double* [B, 9])
//   Norm                  the pair's normalisation, kept in PairState
//   Rows                  a view of the pair's normalised f32 rows in the workspace, passed by value: Row (one row in registers:
//                         what inlier takes), carve (its arrays from the workspace), at(row), row(i, n) (row i, a NaN row for
//                         i >= n) (the two-view models: PairRows, one float4 per row)
//   normalise             every thread of 256: Norm, the Rows (non-finite rows as NaN), squared thresholds, whether the pair
//                         can be sampled
//   hypothesis            the lanes of one hypothesis: its sample's rows from In (the two-view models: load_sample), normalised in
//                         f64, through the minimal solver into the hypothesis' slots (store_model) and Slots::n
//   inlier                the f32 inlier test of one model on one Row; false for a NaN row
//   model_out             the pair's model in the caller's terms (zeros unless good) into Out
// and for MagsacScoring what its comment below lists.
//
// Per pair b (counts[b] rows of the input; later rows are never read):
//   1. ransac_norm_kernel: M::normalise - the model's normalisation, normalised f32 copies of the rows (non-finite rows as
//      NaN), squared thresholds in normalised units, whether the pair can be sampled.  MagsacScoring only:
//      magsac_init_kernel - residual scales, V scale and threshold of the pair.
//   2. rounds of RANSAC_ROUND hypotheses, enqueued ceil(max_iters / ROUND) times, no host synchronisation:
//      ransac_hyp_kernel    M::HYP_LANES lanes per hypothesis: sample (counter-based, from (seed_b, h) only), then
//                           M::hypothesis: its rows normalised in f64, the f64 minimal solver, up to M::SLOTS models
//      ransac_score_kernel  one wave per hypothesis, Sc::score: its models' inlier counts (popc(ballot) of M::inlier, -1 for
//                           unused slots), or their sums of rho (+inf for unused slots) and the counts r < tau
//      ransac_select_kernel per pair: the best key (largest count / smallest sum; ties: lowest (h, slot); an earlier round keeps
//                           a tie), OpenCV's adaptive iteration count from its inlier count, done flag.
//   3. refinement, Sc::steps times (count: M::REFINE_ITERS if M has any and `refine`; MAGSAC++: lo_iters): count only
//      ransac_mask_kernel (inliers of the current model); ransac_refit_kernel (Sc::refit: M::refit, a least-squares candidate on
//      the mask, or M::wrefit, an IRLS step with the MAGSAC++ weights of the current model); ransac_accept_kernel (Sc::accept:
//      the candidate is kept if its inlier count is not lower / its sum of rho strictly lower, else refinement stops).
//   4. ransac_mask_kernel + ransac_finish_kernel: final mask (Sc::inlier), ok flag, M::model_out (model in the caller's terms), info
//      row (write_info, then Sc::finish: MAGSAC++ adds the LO steps and the two scores).
// Every flag and counter of the workspace is written with plain stores by one kernel and read by a later launch on the same
// stream: no atomics and no hand-off inside a launch.  Results are bit-identical from run to run and independent of B.
#pragma once
#include <float.h>
#include <math.h>

#include <algorithm>
#include <string>

#include "common.h"
#include "sampling.h"
#include "workspace.h"

// nothing here is fused: the numpy restatements (tools/geometry_ref.py, tools/essential_ref.py) evaluate the same expressions;
// the scoring is written with explicit fmaf
#pragma clang fp contract(off)

namespace roma {
constexpr int RANSAC_ROUND = 256;  // hypotheses per pair and round (tools/geometry_ref.py: ROUND)

namespace {

constexpr int R = RANSAC_ROUND;
constexpr int MAX_TRY = 64;           // redraws of one sample index before the sample is given up
constexpr double PIVOT_EPS = 1e-6;      // |pivot| of the minimal solvers' elimination (normalised coordinates)

// ------------------------------------------------------------------------------------------------------------ helpers
// Gauss-Jordan elimination with partial pivoting (first maximum) of the pivot columns 0 .. ROWS-1; rows swapped by selects
// so the matrix stays in registers.  false if a pivot is not above PIVOT_EPS in magnitude.
template <int ROWS, int COLS>
__device__ __forceinline__ bool gauss_jordan(double (&a)[ROWS][COLS]) {
#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    int p = k;
    double big = fabs(a[k][k]);
#pragma unroll
    for (int r = k + 1; r < ROWS; ++r) {
      const double v = fabs(a[r][k]);
      if (v > big) { big = v; p = r; }
    }
    if (!(big > PIVOT_EPS)) return false;
#pragma unroll
    for (int r = k + 1; r < ROWS; ++r) {
      const bool sw = r == p;
#pragma unroll
      for (int c = 0; c < COLS; ++c) {
        const double t = a[k][c];
        a[k][c] = sw ? a[r][c] : t;
        a[r][c] = sw ? t : a[r][c];
      }
    }
    const double inv = 1.0 / a[k][k];
#pragma unroll
    for (int c = 0; c < COLS; ++c) a[k][c] = a[k][c] * inv;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if (r == k) continue;
      const double f = a[r][k];
#pragma unroll
      for (int c = 0; c < COLS; ++c) a[r][c] = a[r][c] - f * a[k][c];
    }
  }
  return true;
}

// draw j of hypothesis h: index mix64(key_h + G2 (c + 1)) mod n with c = j, j + S, j + 2S, ... until it differs from the
// draws before it; key_h = mix64(seed + G1 (h + 1)).  Depends on (seed, h) only.
template <int S>
__device__ __forceinline__ bool draw_sample(uint64_t seed, int h, int n, int (&idx)[S]) {
  const uint64_t key = mix64(seed + 0x9e3779b97f4a7c15ull * (uint64_t)(h + 1));
#pragma unroll
  for (int j = 0; j < S; ++j) {
    bool got = false;
    for (int t = 0; t < MAX_TRY && !got; ++t) {
      const uint64_t c = (uint64_t)(j + t * S);
      const int v = (int)(mix64(key + 0xd1b54a32d192ed03ull * (c + 1)) % (uint64_t)n);
      bool dup = false;
#pragma unroll
      for (int k = 0; k < j; ++k) dup |= idx[k] == v;
      if (!dup) {
        idx[j] = v;
        got = true;
      }
    }
    if (!got) return false;
  }
  return true;
}

// OpenCV's RANSACUpdateNumIters with the ceiling of the ratio: hypotheses needed so that, with inlier ratio w, a sample of
// s inliers has been drawn with probability conf
__device__ int update_num_iters(double conf, double w, int s, int max_iters) {
  conf = fmin(fmax(conf, 0.0), 1.0);
  w = fmin(fmax(w, 0.0), 1.0);
  double ws = 1;
  for (int k = 0; k < s; ++k) ws *= w;
  const double num = log(fmax(1 - conf, DBL_MIN));
  double denom = 1 - ws;
  if (denom < DBL_MIN) return 0;
  denom = log(denom);
  if (denom >= 0 || -num >= max_iters * (-denom)) return max_iters;
  return (int)ceil(num / denom);
}

__device__ __forceinline__ double block_sum(double v, double* sh) {  // 256 threads, fixed tree
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] = sh[t] + sh[t + s];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ bool finite_row(float a0, float a1, float b0, float b1) {
  return isfinite(a0) && isfinite(a1) && isfinite(b0) && isfinite(b1);
}

__device__ __forceinline__ void mat3(const double* a, const double* b, double* c) {  // c = a b
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

__device__ __forceinline__ double det3(const double* f) {
  return f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) + f[2] * (f[3] * f[7] - f[4] * f[6]);
}

template <int NM = 9>
__device__ __forceinline__ void to_f32(const double* m, float* mf) {  // the 12-float (three float4) copy the scoring reads
  static_assert(NM <= 12);
#pragma unroll
  for (int k = 0; k < NM; ++k) mf[k] = (float)m[k];
#pragma unroll
  for (int k = NM; k < 12; ++k) mf[k] = 0.f;
}

// ---- symmetric PSD eigenproblems by one-sided (Hestenes) Jacobi on one wave (the refits' 9 x 9 normal equations).  Lane j < NC
// holds column j of M and of V; the P - 1 rounds of the circle method pair every column with every other once per sweep.
// Afterwards the column norms of M V are the eigenvalues and the columns of V the eigenvectors.
constexpr int JACOBI_SWEEPS = 15;
constexpr double JACOBI_TOL = 4 * DBL_EPSILON;

template <int NC, int P>
__device__ __forceinline__ void jacobi_sweeps(double (&a)[NC], double (&v)[NC], int lane) {
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
}

// the eigenvalue of this lane's column (+inf for lanes that hold none)
template <int NC>
__device__ __forceinline__ double jacobi_eigenvalue(const double (&a)[NC], int lane) {
  double nrm = 0;
#pragma unroll
  for (int k = 0; k < NC; ++k) nrm += a[k] * a[k];
  return lane >= NC ? INFINITY : nrm;
}

// smallest eigenvector (lowest lane on ties), on every lane
template <int NC, int P>
__device__ void jacobi_min_vec(double (&a)[NC], double (&v)[NC], int lane, double (&out)[NC]) {
  jacobi_sweeps<NC, P>(a, v, lane);
  double nrm = jacobi_eigenvalue<NC>(a, lane);
  int bl = lane;
  for (int off = 32; off > 0; off >>= 1) {
    const double on = __shfl_xor(nrm, off);
    const int ol = __shfl_xor(bl, off);
    if (on < nrm || (on == nrm && ol < bl)) { nrm = on; bl = ol; }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) out[k] = __shfl(v[k], bl);
}

// ------------------------------------------------------------------------------------------------------------ state, workspace
template <class M>
struct PairState {
  typename M::Norm nrm;         // the model's normalisation of the pair
  double cur[M::NM];            // current model in normalised coordinates
  double cand[M::NM];           // refit candidate
  alignas(16) float curf[12];   // f32 copies the scoring reads
  alignas(16) float candf[12];
  float thr2a, thr2b;           // squared thresholds per image in normalised units
  int n;                        // rows of the pair: counts[b] clamped to [0, N]
  int valid;                    // enough finite rows for a sample, normalisation well defined
  int best;                     // inlier count of the current model (-1: none yet)
  int best_h, best_root, best_min;  // winning minimal sample, its slot and its inlier count
  int needed;                   // adaptive iteration count
  int rounds;                   // rounds executed
  int done;                     // sampling finished for this pair
  int stop;                     // refinement finished for this pair
  int cand_ok;                  // the last refit produced a candidate
};

struct Slots {                  // the models of one round: SLOTS per hypothesis, B * R hypotheses
  double* d;                    // f64 models [B * R * SLOTS][NM]
  float* f;                     // f32 copies [B * R * SLOTS][12]
  int* n;                       // models per hypothesis [B * R]
  int* cnt;                     // inlier count per slot, -1 if unused [B * R * SLOTS]
};

template <int NM = 9>
__device__ __forceinline__ void store_model(const double* m, long slot, const Slots& sl) {
  float mf[12];
  to_f32<NM>(m, mf);
#pragma unroll
  for (int k = 0; k < NM; ++k) sl.d[slot * NM + k] = m[k];
  float4* o = reinterpret_cast<float4*>(sl.f + slot * 12);
  o[0] = make_float4(mf[0], mf[1], mf[2], mf[3]);
  o[1] = make_float4(mf[4], mf[5], mf[6], mf[7]);
  o[2] = make_float4(mf[8], mf[9], mf[10], mf[11]);
}

// ---- In, Rows and the sample load of the two-view models (H, F, E)
struct PairIn {                 // kpts_a, kpts_b [B, N] pixel (E without a camera matrix: normalised) coordinates
  const float2* a;
  const float2* b;
  __device__ PairIn at(long row) const { return {a + row, b + row}; }
};

struct PairRows {               // (xa, ya, xb, yb) normalised, [B * N]
  using Row = float4;
  float4* p;
  static void carve(PairRows& r, Workspace256& ws, size_t rows) { r.p = ws.take<float4>(rows); }
  __device__ PairRows at(long row) const { return {p + row}; }
  __device__ float4 row(int i, int n) const { return i < n ? p[i] : make_float4(NAN, NAN, NAN, NAN); }
};

// rows idx of the pair `in`, normalised in f64; returns whether the sample is usable (it was drawn, and its rows are finite)
template <int S, class Norm>
__device__ __forceinline__ bool load_sample(const PairIn& in, const int (&idx)[S], bool act, const Norm& nrm, double (&xa)[S],
                                            double (&ya)[S], double (&xb)[S], double (&yb)[S]) {
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const float2 a = act ? in.a[idx[k]] : make_float2(0.f, 0.f);
    const float2 q = act ? in.b[idx[k]] : make_float2(0.f, 0.f);
    act = act && finite_row(a.x, a.y, q.x, q.y);
    nrm.apply(a, q, xa[k], ya[k], xb[k], yb[k]);
  }
  return act;
}

template <class M, class Sc>
struct Carve {
  PairState<M>* st;
  typename M::Rows rows;
  Slots sl;
  typename Sc::Ws w;            // what the scoring keeps next to them
  size_t bytes;
};

// the regions of the pipeline, named once: over Workspace256() for the size, over the caller's pointer for the launches
template <class M, class Sc>
Carve<M, Sc> carve(Workspace256 ws, int B, int N) {
  const size_t hyp = (size_t)B * R, slots = hyp * M::SLOTS;
  Carve<M, Sc> c;
  c.st = ws.take<PairState<M>>(B);
  M::Rows::carve(c.rows, ws, (size_t)B * N);
  c.sl.d = ws.take<double>(M::NM * slots);
  c.sl.f = ws.take<float>(12 * slots);
  c.sl.n = ws.take<int>(hyp);
  c.sl.cnt = ws.take<int>(slots);
  Sc::carve(c.w, ws, slots, B);
  c.bytes = ws.bytes();
  return c;
}

template <class M, class Sc>
size_t workspace_bytes(int B, int N) { return B > 0 && N > 0 ? carve<M, Sc>(Workspace256(), B, N).bytes : 0; }

// ------------------------------------------------------------------------------------------------------------ shared by the models
// The f32 scoring of a model is written once, as its residual terms linear in the model (Model::res_terms, NT of them): the
// count scoring's inlier test (Model::inlier_from) and the MAGSAC++ squared residual (Model::r2_from) are both formed from them,
// and the MAGSAC++ accept step evaluates a candidate as current + difference on the same terms.
template <class Model>
struct Terms {
  __device__ static bool inlier(const float* m, float4 p, float t2a, float t2b) {
    float t[Model::NT];
    Model::res_terms(m, p, t);
    return Model::inlier_from(t, t2a, t2b);
  }
  __device__ static float residual2(const float* m, float4 p, float sa2, float sb2) {
    float t[Model::NT];
    Model::res_terms(m, p, t);
    return Model::r2_from(t, sa2, sb2);
  }
};

// the epipolar terms of F and E: (d, l_x, l_y, k_x, k_y) with d = x_b^T M x_a, l = M x_a, k = M^T x_b; p = (xa, ya, xb, yb)
__device__ __forceinline__ void epipolar_terms(const float* m, float4 p, float (&t)[5]) {
  const float lx = fmaf(m[0], p.x, fmaf(m[1], p.y, m[2]));
  const float ly = fmaf(m[3], p.x, fmaf(m[4], p.y, m[5]));
  const float lz = fmaf(m[6], p.x, fmaf(m[7], p.y, m[8]));
  t[0] = fmaf(p.z, lx, fmaf(p.w, ly, lz));
  t[1] = lx;
  t[2] = ly;
  t[3] = fmaf(m[0], p.z, fmaf(m[3], p.w, m[6]));
  t[4] = fmaf(m[1], p.z, fmaf(m[4], p.w, m[7]));
}

// the info row every model shares: {rounds, best_h, best_root, [best_min,] best, valid}; returns the entries written
template <class M>
__device__ __forceinline__ int write_info(const PairState<M>& P, int* info, bool with_min) {
  int k = 0;
  info[k++] = P.rounds;
  info[k++] = P.best_h;
  info[k++] = P.best_root;
  if (with_min) info[k++] = P.best_min;
  info[k++] = P.best;
  info[k++] = P.valid;
  return k;
}
constexpr int INFO_CORE = 5;    // the entries of write_info without best_min

// Hartley normalisation (centroid to 0, mean distance to sqrt 2) of both images over the rows that `row` selects, every thread
// of the 256: row(i, ax, ay, bx, by) -> whether row i counts, and its coordinates.  f64 sums in a fixed order (block_sum).
struct HartleyMoments {
  double cnt, cax, cay, cbx, cby, ma, mb, sa, sb;  // rows, centroids, mean distances, scales x_n = (x - c) s
  __device__ bool ok(int rows) const { return cnt >= rows && ma > 0 && mb > 0 && isfinite(sa) && isfinite(sb); }
};

template <class Row>
__device__ __forceinline__ HartleyMoments hartley_moments(int n, Row row, double* sh) {
  const int t = threadIdx.x;
  HartleyMoments m;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (int i = t; i < n; i += 256) {
    double ax, ay, bx, by;
    if (row(i, ax, ay, bx, by)) { s0 += ax; s1 += ay; s2 += bx; s3 += by; s4 += 1; }
  }
  m.cnt = block_sum(s4, sh);
  m.cax = block_sum(s0, sh) / m.cnt;
  m.cay = block_sum(s1, sh) / m.cnt;
  m.cbx = block_sum(s2, sh) / m.cnt;
  m.cby = block_sum(s3, sh) / m.cnt;
  double da = 0, db = 0;
  for (int i = t; i < n; i += 256) {
    double ax, ay, bx, by;
    if (row(i, ax, ay, bx, by)) {
      ax = ax - m.cax; ay = ay - m.cay; bx = bx - m.cbx; by = by - m.cby;
      da += sqrt(ax * ax + ay * ay);
      db += sqrt(bx * bx + by * by);
    }
  }
  m.ma = block_sum(da, sh) / m.cnt;
  m.mb = block_sum(db, sh) / m.cnt;
  m.sa = M_SQRT2 / m.ma;
  m.sb = M_SQRT2 / m.mb;
  return m;
}

// The refits' 9 x 9 normal equations, every thread of the 256: sum over the rows i < n that `sel` selects of w a a^T (TWO: of
// w (a a^T + a2 a2^T), the homography's two rows per point); sel(i, w) -> whether row i counts, and its weight (read only if W);
// row(i, a, a2) -> its row(s), called for selected rows only (on its own, so that the constants of a row reach the products).
// Per thread in ascending i, then over the wave by a fixed butterfly, over the four waves in order, and symmetrised into Mx;
// returns the number of rows selected.  Mx is published (the barrier is the last thing here).
template <bool W, bool TWO, class Sel, class Row>
__device__ __forceinline__ int normal_equations(int n, Sel sel, Row row, double (&Mx)[9][9]) {
  __shared__ double red[4][45];
  __shared__ int cnt[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double acc[45];
#pragma unroll
  for (int e = 0; e < 45; ++e) acc[e] = 0;
  int rows = 0;
  for (int i = t; i < n; i += 256) {
    double wt = 1;
    if (!sel(i, wt)) continue;
    ++rows;
    double a[9], a2[9];
    row(i, a, a2);
    int e = 0;
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
      for (int q = p; q < 9; ++q, ++e) {
        if constexpr (TWO) {
          if constexpr (W) acc[e] += wt * (a[p] * a[q] + a2[p] * a2[q]);
          else acc[e] += a[p] * a[q] + a2[p] * a2[q];
        } else {
          if constexpr (W) acc[e] += wt * (a[p] * a[q]);
          else acc[e] += a[p] * a[q];
        }
      }
  }
  for (int off = 32; off > 0; off >>= 1) rows += __shfl_xor(rows, off);
  if (lane == 0) cnt[wave] = rows;
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
    const int q = p + e;
    const double s = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    Mx[p][q] = s;
    Mx[q][p] = s;
  }
  rows = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
  __syncthreads();
  return rows;
}

// ------------------------------------------------------------------------------------------------------------ MAGSAC++ arithmetic
// MAGSAC++ (Barath et al., CVPR 2020; nu = 4; tools/magsac_ref.py restates it): a model's score is the sum over the pair's rows
// of the loss rho(V), V = r^2 k^2 / (2 tau^2) with r the model's residual (M::residual2) and tau the threshold (M::mag_thr2:
// both in the model's own units - pixels for H and F, normalised camera coordinates for E); lower is better.
constexpr double MAGSAC_K2 = 13.276704135987625;      // 0.99 quantile of chi^2 with 4 DoF
constexpr float MAGSAC_VK = 6.638352067993813f;       // k^2 / 2
constexpr float MAGSAC_GK = 0.003611260617758621f;    // Gamma(3/2, V_k)
constexpr float MAGSAC_RHO_MAX = 1.3015316073311316f; // gamma(5/2, V_k): the loss of an outlier and of a non-finite row
constexpr float HALF_SQRT_PI = 0.886226925452758f;    // Gamma(3/2)

// rho(V) = gamma(5/2, V) + V (Gamma(3/2, V) - Gamma(3/2, V_k)) and w(V) = Gamma(3/2, V) - Gamma(3/2, V_k) for V < V_k; (RHO_MAX, 0)
// beyond and for NaN.  Gamma(3/2, V) = sqrt(pi) / 2 erfc(sqrt V) + sqrt(V) e^-V, gamma(3/2, V) = Gamma(3/2) - Gamma(3/2, V),
// gamma(5/2, V) = 3/2 gamma(3/2, V) - V^{3/2} e^-V.
__device__ __forceinline__ float magsac_rho(float V, float& w) {
  if (!(V < MAGSAC_VK)) {
    w = 0.f;
    return MAGSAC_RHO_MAX;
  }
  const float s = sqrtf(V), se = s * expf(-V);
  const float G = fmaf(HALF_SQRT_PI, erfcf(s), se);
  const float g52 = fmaf(1.5f, HALF_SQRT_PI - G, -(V * se));
  w = G - MAGSAC_GK;
  return fmaf(V, w, g52);
}

struct MagState {               // per pair, next to PairState
  float sa2, sb2;               // squared normalisation scales M::residual2 divides by
  float vs;                     // k^2 / (2 tau^2): V = r^2 vs
  float t2;                     // tau^2: inlier r^2 < t2
  float score;                  // sum of rho of the running best of the sampling rounds (+inf: none yet)
  float score_min;              // sum of rho of the winning minimal model
  int lo_steps;                 // LO steps accepted
  double gain;                  // what the accepted LO steps lowered the sum of rho by (MagsacScoring::accept)
};

// s + x with its rounding error added to the compensation c (Knuth's TwoSum: exact, whatever the order of s and x)
__device__ __forceinline__ void two_sum(float& s, float& c, float x) {
  const float t = s + x, bp = t - s;
  c += (s - (t - bp)) + (x - bp);
  s = t;
}

// the wave's total of the lanes' compensated sums (s, c): a fixed butterfly; both lanes of a pair compute the same
// (sum, compensation), so every lane ends with the same value
__device__ __forceinline__ float wave_total(float s, float c) {
  for (int off = 32; off > 0; off >>= 1) {
    const float so = __shfl_xor(s, off), co = __shfl_xor(c, off);
    c = c + co;
    two_sum(s, c, so);
  }
  return s + c;
}

// one wave: sum of rho of SL models (wave-uniform coefficients mf, the first nm used) over rows 0 .. n-1, and their inlier counts.
// Compensated f32 sums (TwoSum): a plain f32 sum of thousands of rows resolves no change below ~1e-7 of the total, which is
// larger than what a late IRLS step gains, and LO would stop on rounding.
template <class M, int SL>
__device__ __forceinline__ void magsac_sums(const float* mf, int nm, const float4* __restrict__ Pp, int n, const MagState& S,
                                            int lane, float (&acc)[SL], int (&c)[SL]) {
  const float sa2 = S.sa2, sb2 = S.sb2, vs = S.vs, t2 = S.t2;
  float cmp[SL];
#pragma unroll
  for (int r = 0; r < SL; ++r) { acc[r] = 0.f; cmp[r] = 0.f; c[r] = 0; }
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool row = i < n;
    const float4 p = row ? Pp[i] : make_float4(NAN, NAN, NAN, NAN);
#pragma unroll
    for (int r = 0; r < SL; ++r) {
      if (M::SCORE_EVERY_SLOT || r < nm) {
        const float r2 = M::residual2(mf + 12 * r, p, sa2, sb2);
        c[r] += __popcll(__ballot(r2 < t2));
        float w;
        const float rho = magsac_rho(r2 * vs, w);
        two_sum(acc[r], cmp[r], row ? rho : 0.f);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < SL; ++r) acc[r] = wave_total(acc[r], cmp[r]);
}

// lane 0 of the accept wave: the candidate (c inliers) becomes the current model, or refinement stops
template <class M>
__device__ __forceinline__ void settle(PairState<M>& P, bool keep, int c) {
  if (keep) {
    P.best = c;
    for (int k = 0; k < M::NM; ++k) P.cur[k] = P.cand[k];
    for (int k = 0; k < 12; ++k) P.curf[k] = P.candf[k];
  } else {
    P.stop = 1;
  }
  P.cand_ok = 0;
}

// ------------------------------------------------------------------------------------------------------------ scoring policies
// What a scoring supplies to the pipeline below: Ws (what it keeps in the workspace next to the pair states) and carve; Key,
// worst, better, keys, running and record (the arg-best of the select kernel); score (what one wave computes for one hypothesis,
// and stores per slot); inlier (the mask); refit and accept (one refinement step), REFITS, steps and MASK_BEFORE_REFIT (whether
// and how often the host enqueues it, from the entry point's `refine` / `lo_iters`); INFO, INFO_MIN and finish (its info row);
// INIT (a launch that fills Ws) and SCORES (the entry point has an out_score).

// Inlier counts: larger is better; refinement is a least-squares refit on the current inliers, kept while the count does not drop.
struct CountScoring {
  using Key = int;
  struct Ws {};                 // nothing: the keys are Slots::cnt, the running best PairState::best
  static constexpr bool INIT = false, MASK_BEFORE_REFIT = true, SCORES = false;
  static constexpr int MAX_STEPS = 0;  // `refine` is a flag
  template <class M> static constexpr int INFO = M::INFO;
  template <class M> static constexpr bool INFO_MIN = M::INFO > INFO_CORE;
  template <class M> static constexpr bool REFITS = M::REFINE_ITERS > 0;
  template <class M> static int steps(int refine) { return refine ? M::REFINE_ITERS : 0; }
  static void carve(Ws&, Workspace256&, size_t, int) {}

  __device__ static Key worst() { return -1; }
  __device__ static bool better(Key a, Key b) { return a > b; }
  __device__ static const Key* keys(const Ws&, const Slots& sl) { return sl.cnt; }
  template <class M> __device__ static Key running(const PairState<M>& P, const Ws&, int) { return P.best; }
  __device__ static void record(const Ws&, int, Key) {}

  // the models' f32 inlier tests (M::inlier), popc(ballot) counts, -1 for unused slots
  template <class M>
  __device__ static void score(const float* mf, int nm, typename M::Rows rows, const PairState<M>& P, const Ws&, int, int lane,
                               long g, const Slots& sl) {
    constexpr int SL = M::SLOTS;
    const int n = P.n;
    const float t2a = P.thr2a, t2b = P.thr2b;
    int c[SL];
#pragma unroll
    for (int r = 0; r < SL; ++r) c[r] = 0;
    if (nm > 0) {
      for (int i0 = 0; i0 < n; i0 += 64) {
        const typename M::Rows::Row p = rows.row(i0 + lane, n);
#pragma unroll
        for (int r = 0; r < SL; ++r)
          if (M::SCORE_EVERY_SLOT || r < nm) c[r] += __popcll(__ballot(M::inlier(mf + 12 * r, p, t2a, t2b)));
      }
    }
    if (lane == 0) {
      int* o = sl.cnt + g * SL;
#pragma unroll
      for (int r = 0; r < SL; ++r) o[r] = r < nm ? c[r] : -1;
    }
  }

  template <class M>
  __device__ static bool inlier(const PairState<M>& P, const Ws&, int, typename M::Rows::Row p) {
    return M::inlier(P.curf, p, P.thr2a, P.thr2b);
  }

  template <class M>
  __device__ static void refit(const float2* A, const float2* Bp, const float4*, PairState<M>& P, const Ws&, int,
                               const unsigned char* mask) {
    M::refit(A, Bp, P, mask);
  }

  // re-score the candidate; keep it if its count is not lower, else stop refining
  template <class M>
  __device__ static void accept(typename M::Rows rows, PairState<M>& P, const Ws&, int, int lane) {
    const int n = P.n;
    const float t2a = P.thr2a, t2b = P.thr2b;
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += 64)
      c += __popcll(__ballot(M::inlier(P.candf, rows.row(i0 + lane, n), t2a, t2b)));
    if (lane == 0) settle(P, c >= P.best, c);
  }

  template <class M>
  __device__ static void finish(const PairState<M>&, const Ws&, int, int*, double*) {}
};

// MAGSAC++: the key is the sum of rho, smaller is better, the inlier count r < tau carried along for the adaptive iteration
// count; refinement is IRLS local optimisation (M::wrefit), a step kept only if it lowers the sum of rho.  From the model it
// needs residual2 / res_terms / r2_from / NT, res_scales, mag_thr2, wrefit, MAG_INFO, and it is written for the two-view models:
// Rows = PairRows, In = PairIn, NM = 9.
struct MagsacScoring {
  using Key = float;
  struct Ws {
    MagState* ms;               // [B]
    float* sc;                  // sum of rho per slot, +inf if unused [B * R * SLOTS]
  };
  static constexpr bool INIT = true, MASK_BEFORE_REFIT = false, SCORES = true;
  static constexpr int MAX_STEPS = 64;  // lo_iters of the entry points (MAGSAC_MAX_LO, ESSENTIAL_MAGSAC_MAX_LO)
  template <class M> static constexpr int INFO = M::MAG_INFO;
  template <class M> static constexpr bool INFO_MIN = true;
  template <class M> static constexpr bool REFITS = true;
  template <class M> static int steps(int lo_iters) { return lo_iters; }
  static void carve(Ws& w, Workspace256& ws, size_t slots, int B) {
    w.ms = ws.take<MagState>(B);
    w.sc = ws.take<float>(slots);
  }

  __device__ static Key worst() { return INFINITY; }
  __device__ static bool better(Key a, Key b) { return a < b; }
  __device__ static const Key* keys(const Ws& w, const Slots&) { return w.sc; }
  template <class M> __device__ static Key running(const PairState<M>&, const Ws& w, int b) { return w.ms[b].score; }
  __device__ static void record(const Ws& w, int b, Key v) {
    w.ms[b].score = v;
    w.ms[b].score_min = v;
  }

  // one thread per pair (magsac_init_kernel): residual scales, V scale, threshold (M::mag_thr2: tau^2 in the units of M::residual2)
  template <class M>
  __device__ static void init(const PairState<M>& P, float thr, MagState& S) {
    M::res_scales(P.nrm, S.sa2, S.sb2);
    const double t2 = M::mag_thr2(P.nrm, thr);
    S.vs = (float)(MAGSAC_K2 / (2 * t2));
    S.t2 = (float)t2;
    S.score = INFINITY;
    S.score_min = INFINITY;
    S.lo_steps = 0;
    S.gain = 0.0;
  }

  // compensated f32 sum of rho per slot (lane partials over rows i = lane mod 64 ascending, then a fixed butterfly), and the
  // count r < tau
  template <class M>
  __device__ static void score(const float* mf, int nm, PairRows rows, const PairState<M>& P, const Ws& w, int b, int lane, long g,
                               const Slots& sl) {
    constexpr int SL = M::SLOTS;
    float acc[SL];
    int c[SL];
#pragma unroll
    for (int r = 0; r < SL; ++r) { acc[r] = 0.f; c[r] = 0; }
    if (nm > 0) magsac_sums<M, SL>(mf, nm, rows.p, P.n, w.ms[b], lane, acc, c);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < SL; ++r) {
        w.sc[g * SL + r] = r < nm ? acc[r] : INFINITY;
        sl.cnt[g * SL + r] = r < nm ? c[r] : -1;
      }
    }
  }

  template <class M>
  __device__ static bool inlier(const PairState<M>& P, const Ws& w, int b, float4 p) {  // r < tau
    const MagState& S = w.ms[b];
    return M::residual2(P.curf, p, S.sa2, S.sb2) < S.t2;
  }

  template <class M>
  __device__ static void refit(const float2* A, const float2* Bp, const float4* pts, PairState<M>& P, const Ws& w, int b,
                               const unsigned char*) {
    M::wrefit(A, Bp, pts, P, w.ms[b]);
  }

  // keep the candidate if its sum of rho is strictly lower than the current model's, else stop.  The gain sum(rho_cur - rho_cand)
  // is measured on the same rows in one pass, the candidate's residual terms as the current model's plus those of the f32
  // difference (cand - cur): rounding the two models to f32 separately moves each sum by far more than a late IRLS step gains (an
  // inlier's residual is a small difference of O(1) normalised terms), and paired this way the shared part of that error
  // cancels.  The inlier count is the candidate's own (what the mask kernel evaluates).
  template <class M>
  __device__ static void accept(PairRows rows, PairState<M>& P, const Ws& w, int b, int lane) {
    constexpr int NT = M::NT;
    const float4* __restrict__ Pp = rows.p;
    MagState& S = w.ms[b];
    float dm[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) dm[k] = (float)(P.cand[k] - P.cur[k]);
    const int n = P.n;
    const float sa2 = S.sa2, sb2 = S.sb2, vs = S.vs, t2 = S.t2;
    float g = 0.f, gc = 0.f;
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const bool row = i < n;
      const float4 p = row ? Pp[i] : make_float4(NAN, NAN, NAN, NAN);
      float tu[NT], td[NT], tc[NT];
      M::res_terms(P.curf, p, tu);
      M::res_terms(dm, p, td);
#pragma unroll
      for (int k = 0; k < NT; ++k) tc[k] = tu[k] + td[k];
      float wt;
      const float ru = magsac_rho(M::r2_from(tu, sa2, sb2) * vs, wt);
      const float rc = magsac_rho(M::r2_from(tc, sa2, sb2) * vs, wt);
      two_sum(g, gc, row ? ru - rc : 0.f);
      c += __popcll(__ballot(M::residual2(P.candf, p, sa2, sb2) < t2));
    }
    g = wave_total(g, gc);
    if (lane == 0) {
      if (g > 0.f) {
        S.gain = S.gain + (double)g;
        S.lo_steps = S.lo_steps + 1;
      }
      settle(P, g > 0.f, c);
    }
  }

  // LO steps after the shared info entries; scores (the final sum of rho is the winning minimal model's less the gains of the
  // accepted LO steps)
  template <class M>
  __device__ static void finish(const PairState<M>& P, const Ws& w, int b, int* info, double* score) {
    const MagState& S = w.ms[b];
    info[0] = S.lo_steps;
    const bool found = P.best_h >= 0;
    score[2 * (long)b] = found ? (double)S.score_min : 0.0;
    score[2 * (long)b + 1] = found ? (double)S.score_min - S.gain : 0.0;
  }
};

// ------------------------------------------------------------------------------------------------------------ kernels
template <class M>
__global__ __launch_bounds__(256) void ransac_norm_kernel(typename M::In in, const int* __restrict__ counts,
                                                          const double* __restrict__ K, int N, float thr, int max_iters,
                                                          PairState<M>* __restrict__ st, typename M::Rows rows) {
  __shared__ double sh[256];
  const int b = blockIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  typename M::Norm nrm;
  float t2a, t2b;
  const bool valid = M::normalise(in.at((long)b * N), n, K ? K + (long)b * 9 : nullptr, thr, sh, rows.at((long)b * N), nrm, t2a, t2b);
  if (threadIdx.x == 0) {
    PairState<M>& S = st[b];
    S.nrm = nrm;
    S.thr2a = t2a;
    S.thr2b = t2b;
    S.n = n;
    S.valid = valid ? 1 : 0;
    S.best = -1; S.best_h = -1; S.best_root = -1; S.best_min = -1;
    S.needed = max_iters;
    S.rounds = 0;
    S.done = valid ? 0 : 1;
    S.stop = 0;
    S.cand_ok = 0;
    for (int k = 0; k < M::NM; ++k) { S.cur[k] = 0; S.cand[k] = 0; }
    for (int k = 0; k < 12; ++k) { S.curf[k] = 0; S.candf[k] = 0; }
  }
}

// one thread per pair: the MAGSAC++ state of the pair (MagsacScoring::init)
template <class M>
__global__ __launch_bounds__(64) void magsac_init_kernel(int B, float thr, const PairState<M>* __restrict__ st,
                                                         MagState* __restrict__ ms) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  MagsacScoring::init<M>(st[b], thr, ms[b]);
}

// HYP_LANES lanes per (pair, hypothesis of the round), HYP_THREADS per workgroup; grid B * R * HYP_LANES / HYP_THREADS
template <class M>
__global__ __launch_bounds__(M::HYP_THREADS) void ransac_hyp_kernel(typename M::In in, int N,
                                                                    const unsigned long long* __restrict__ seeds,
                                                                    const PairState<M>* __restrict__ st, int round, Slots sl) {
  constexpr int S = M::S, L = M::HYP_LANES;
  static_assert(R % (M::HYP_THREADS / L) == 0, "a workgroup must not straddle two pairs");
  const int g = blockIdx.x * (M::HYP_THREADS / L) + threadIdx.x / L, b = g / R;
  const PairState<M>& P = st[b];
  if (P.done) return;  // uniform over the workgroup: its hypotheses belong to one pair
  const int h = round * R + g % R;
  int idx[S];
  const bool act = draw_sample<S>(seeds[b], h, P.n, idx);
  M::hypothesis(in.at((long)b * N), idx, act, P.nrm, g, threadIdx.x % L, sl);
}

// one wave per (pair, hypothesis): the hypothesis' models (wave-uniform coefficients) against the pair's points (Sc::score)
template <class M, class Sc>
__global__ __launch_bounds__(256) void ransac_score_kernel(typename M::Rows rows, int N, const PairState<M>* __restrict__ st,
                                                           typename Sc::Ws w, Slots sl) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = g / R;
  const PairState<M>& P = st[b];
  if (P.done) return;
  Sc::template score<M>(sl.f + (long)g * M::SLOTS * 12, sl.n[g], rows.at((long)b * N), P, w, b, lane, g, sl);
}

// one workgroup per pair: best key of the round (ties: lowest (h, slot)), running best, adaptive iteration count, done flag
template <class M, class Sc>
__global__ __launch_bounds__(256) void ransac_select_kernel(PairState<M>* __restrict__ st, typename Sc::Ws w, int round, double conf,
                                                            int max_iters, Slots sl) {
  using Key = typename Sc::Key;
  constexpr int SL = M::SLOTS;
  __shared__ Key sk[256];
  __shared__ int si[256];
  const int b = blockIdx.x, t = threadIdx.x;
  PairState<M>& P = st[b];
  if (P.done) return;
  const Key* key = Sc::keys(w, sl) + (long)b * R * SL;
  Key bk = Sc::worst();
  int bi = 0x7fffffff;
  for (int k = t; k < R * SL; k += 256) {
    const Key v = key[k];
    if (Sc::better(v, bk)) { bk = v; bi = k; }  // k ascends: ties keep the lower slot
  }
  sk[t] = bk;
  si[t] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const Key v = sk[t + s];
      const int i = si[t + s];
      if (Sc::better(v, sk[t]) || (v == sk[t] && i < si[t])) { sk[t] = v; si[t] = i; }
    }
    __syncthreads();
  }
  if (t == 0) {
    const Key v = sk[0];
    const int k = si[0];
    if (Sc::better(v, Sc::template running<M>(P, w, b))) {  // strictly: an earlier round's model keeps a tie
      Sc::record(w, b, v);
      const int c = sl.cnt[(long)b * R * SL + k];
      P.best = c;
      P.best_min = c;
      P.best_h = round * R + k / SL;
      P.best_root = k % SL;
      const double* m = sl.d + ((long)b * R * SL + k) * M::NM;
      for (int q = 0; q < M::NM; ++q) P.cur[q] = m[q];
      to_f32<M::NM>(P.cur, P.curf);
      P.needed = update_num_iters(conf, (double)c / P.n, M::S, max_iters);
    }
    P.rounds = round + 1;
    const long drawn = (long)(round + 1) * R;
    P.done = drawn >= (long)min(max_iters, P.needed) ? 1 : 0;
  }
}

// mask[b, i] = inlier of the current model (Sc::inlier; rows beyond counts[b], and pairs without a model: 0); grid (ceil(N / 256), B).
// A pair that is not valid needs no test of its own: it starts with done = 1, so no round touches it and its best stays -1.
template <class M, class Sc>
__global__ __launch_bounds__(256) void ransac_mask_kernel(typename M::Rows rows, int N, const PairState<M>* __restrict__ st,
                                                          typename Sc::Ws w, unsigned char* __restrict__ mask) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const PairState<M>& P = st[b];
  bool in = false;
  if (P.best >= M::MIN_INLIERS && i < P.n) in = Sc::template inlier<M>(P, w, b, rows.at((long)b * N).row(i, P.n));
  mask[(long)b * N + i] = in ? 1 : 0;
}

// one workgroup per pair: a candidate from the current model (Sc::refit: M::refit on the mask, or M::wrefit)
template <class M, class Sc>
__global__ __launch_bounds__(256) void ransac_refit_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb,
                                                           const float4* __restrict__ pts, int N, PairState<M>* __restrict__ st,
                                                           typename Sc::Ws w, const unsigned char* __restrict__ mask) {
  const int b = blockIdx.x;
  const long o = (long)b * N;
  Sc::template refit<M>(ka + o, kb + o, pts + o, st[b], w, b, mask + o);
}

// one wave per pair: re-score the candidate and keep it or stop (Sc::accept)
template <class M, class Sc>
__global__ __launch_bounds__(64) void ransac_accept_kernel(typename M::Rows rows, int N, PairState<M>* __restrict__ st,
                                                           typename Sc::Ws w) {
  const int b = blockIdx.x, lane = threadIdx.x;
  PairState<M>& P = st[b];
  if (P.stop || !P.cand_ok) return;
  Sc::template accept<M>(rows.at((long)b * N), P, w, b, lane);
}

// one thread per pair: ok flag, M::model_out (model in the caller's terms), the info row (write_info, then Sc::finish), Sc's scores
template <class M, class Sc>
__global__ __launch_bounds__(64) void ransac_finish_kernel(int B, const PairState<M>* __restrict__ st, typename Sc::Ws w,
                                                           typename M::Out out, unsigned char* __restrict__ ok,
                                                           int* __restrict__ info, double* __restrict__ score) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const PairState<M>& P = st[b];
  const bool good = P.valid && P.best >= M::MIN_INLIERS;
  M::model_out(P, good, out, b);
  int* row = info + (long)b * Sc::template INFO<M>;
  Sc::template finish<M>(P, w, b, row + write_info(P, row, Sc::template INFO_MIN<M>), score);
  ok[b] = good ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ host
// the argument checks of every entry point: `op` prefixes each message, `conf` names the confidence argument, `opt` is `refine`
// or `lo_iters` (Sc::MAX_STEPS bounds the latter)
template <class Sc>
int check_args(const char* op, const char* conf, bool pointers, int B, int N, float threshold, double confidence, int max_iters,
               int opt, size_t ws_bytes, size_t ws_need) {
  const std::string o(op);
  ROMA_REQUIRE(pointers, o + ": null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16), o + ": need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(max_iters > 0, o + ": max_iters must be positive");
  ROMA_REQUIRE(threshold > 0 && isfinite(threshold), o + ": threshold must be positive and finite");
  ROMA_REQUIRE(confidence >= 0 && confidence <= 1, o + ": " + conf + " must lie in [0, 1]");
  ROMA_REQUIRE(ws_bytes >= ws_need, o + ": workspace too small (roma_op_" + o + "_workspace)");
  if constexpr (Sc::MAX_STEPS > 0)
    ROMA_REQUIRE(opt >= 0 && opt <= Sc::MAX_STEPS, o + ": lo_iters must lie in [0, " + std::to_string(Sc::MAX_STEPS) + "]");
  return 0;
}

// the launch sequence of the pipeline; in, out_model: the model's input and output arrays (M::In, M::Out); K: [B, 3, 3] f64 camera
// matrices or NULL, read by M::normalise only; opt: the entry point's `refine` or `lo_iters` (Sc::steps); out_score: NULL for a
// scoring without scores.  The refit kernel is launched for the two-view models only and takes their arrays.
template <class M, class Sc>
int ransac_run(typename M::In in, const int* counts, const unsigned long long* seeds, const double* K, int B, int N, float thr,
               double conf, int max_iters, int opt, typename M::Out out_model, unsigned char* out_mask, unsigned char* out_ok,
               int* out_info, double* out_score, void* ws, hipStream_t s) {
  const Carve<M, Sc> c = carve<M, Sc>(Workspace256(ws), B, N);
  hipLaunchKernelGGL(ransac_norm_kernel<M>, dim3(B), dim3(256), 0, s, in, counts, K, N, thr, max_iters, c.st, c.rows);
  ROMA_LAUNCH_CHECK();
  if constexpr (Sc::INIT) {
    hipLaunchKernelGGL(magsac_init_kernel<M>, dim3((B + 63) / 64), dim3(64), 0, s, B, thr, c.st, c.w.ms);
    ROMA_LAUNCH_CHECK();
  }
  const int rounds = (max_iters + R - 1) / R;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(ransac_hyp_kernel<M>, dim3(B * R * M::HYP_LANES / M::HYP_THREADS), dim3(M::HYP_THREADS), 0, s, in, N, seeds,
                       c.st, r, c.sl);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL((ransac_score_kernel<M, Sc>), dim3(B * R / 4), dim3(256), 0, s, c.rows, N, c.st, c.w, c.sl);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL((ransac_select_kernel<M, Sc>), dim3(B), dim3(256), 0, s, c.st, c.w, r, conf, max_iters, c.sl);
    ROMA_LAUNCH_CHECK();
  }
  const dim3 mgrid((N + 255) / 256, B);
  if constexpr (Sc::template REFITS<M>) {
    for (int it = 0, n = Sc::template steps<M>(opt); it < n; ++it) {
      if (Sc::MASK_BEFORE_REFIT) {
        hipLaunchKernelGGL((ransac_mask_kernel<M, Sc>), mgrid, dim3(256), 0, s, c.rows, N, c.st, c.w, out_mask);
        ROMA_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL((ransac_refit_kernel<M, Sc>), dim3(B), dim3(256), 0, s, in.a, in.b, c.rows.p, N, c.st, c.w, out_mask);
      ROMA_LAUNCH_CHECK();
      hipLaunchKernelGGL((ransac_accept_kernel<M, Sc>), dim3(B), dim3(64), 0, s, c.rows, N, c.st, c.w);
      ROMA_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL((ransac_mask_kernel<M, Sc>), mgrid, dim3(256), 0, s, c.rows, N, c.st, c.w, out_mask);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL((ransac_finish_kernel<M, Sc>), dim3((B + 63) / 64), dim3(64), 0, s, B, c.st, c.w, out_model, out_ok, out_info,
                     out_score);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace roma
