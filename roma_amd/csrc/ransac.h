// Batched RANSAC on the device: one pipeline for every model, templated on a model policy M (geometry.hip: homography and
// fundamental matrix; essential.hip: essential matrix).  tools/geometry_ref.py restates it in numpy float64 (round_loop) and
// is, with the models' own restatements, the oracle of the GPU tests.
//
// Per pair b (counts[b] rows of kpts_a / kpts_b; later rows are never read):
//   1. ransac_norm_kernel: M::normalise - the model's normalisation of both images, normalised f32 copies of the points
//      (non-finite rows as NaN), squared thresholds in normalised units, whether the pair can be sampled.
//   2. rounds of RANSAC_ROUND hypotheses, enqueued ceil(max_iters / ROUND) times, no host synchronisation:
//      ransac_hyp_kernel    M::HYP_LANES lanes per hypothesis: sample (counter-based, from (seed_b, h) only), normalised in
//                           f64 (M::Norm::apply), then M::hypothesis: the f64 minimal solver, up to M::SLOTS models
//      ransac_score_kernel  one wave per hypothesis: its models' f32 inlier tests (M::inlier), popc(ballot) counts, -1 for
//                           unused slots
//      ransac_select_kernel per pair: arg-max (ties: lowest (h, slot)), OpenCV's adaptive iteration count, done flag.
//   3. refinement (M::REFINE_ITERS > 0 and refine): up to REFINE_ITERS times ransac_mask_kernel (inliers of the current
//      model), ransac_refit_kernel (M::refit: a least-squares candidate), ransac_accept_kernel (re-score; the candidate is kept
//      if its inlier count is not lower, else refinement stops).
//   4. ransac_mask_kernel + ransac_finish_kernel: final mask, ok flag, M::finish (model in pixel terms, info row).
// magsac_run (below) is the same pipeline with MAGSAC++ scoring and IRLS local optimisation (tools/magsac_ref.py for H and F,
// tools/essential_magsac_ref.py for E).
// Every flag and counter of the workspace is written with plain stores by one kernel and read by a later launch on the same
// stream: no atomics and no hand-off inside a launch.  Results are bit-identical from run to run and independent of B.
#pragma once
#include <float.h>
#include <math.h>

#include <algorithm>
#include <string>

#include "common.h"
#include "sampling.h"

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

__device__ __forceinline__ void to_f32(const double* m, float* mf) {  // the 12-float (three float4) copy the scoring reads
#pragma unroll
  for (int k = 0; k < 9; ++k) mf[k] = (float)m[k];
#pragma unroll
  for (int k = 9; k < 12; ++k) mf[k] = 0.f;
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
  double cur[9];                // current model in normalised coordinates
  double cand[9];               // refit candidate
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
  double* d;                    // f64 models [B * R * SLOTS][9]
  float* f;                     // f32 copies [B * R * SLOTS][12]
  int* n;                       // models per hypothesis [B * R]
  int* cnt;                     // inlier count per slot, -1 if unused [B * R * SLOTS]
};

__device__ __forceinline__ void store_model(const double* m, long slot, const Slots& sl) {
  float mf[12];
  to_f32(m, mf);
#pragma unroll
  for (int k = 0; k < 9; ++k) sl.d[slot * 9 + k] = m[k];
  float4* o = reinterpret_cast<float4*>(sl.f + slot * 12);
  o[0] = make_float4(mf[0], mf[1], mf[2], mf[3]);
  o[1] = make_float4(mf[4], mf[5], mf[6], mf[7]);
  o[2] = make_float4(mf[8], mf[9], mf[10], mf[11]);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

template <typename T>
T align_base(void* ws) {  // the caller's workspace need not be 256-aligned: every carve keeps 256 bytes of slack
  return reinterpret_cast<T>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255);
}

template <class M>
struct Carve {
  PairState<M>* st;
  float4* pts;
  Slots sl;
  size_t bytes;
};

template <class M>
Carve<M> carve(void* ws, int B, int N) {
  constexpr int SL = M::SLOTS;
  Carve<M> c;
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  c.st = reinterpret_cast<PairState<M>*>(p + o); o = align256(o + sizeof(PairState<M>) * B);
  c.pts = reinterpret_cast<float4*>(p + o); o = align256(o + sizeof(float4) * (size_t)B * N);
  c.sl.d = reinterpret_cast<double*>(p + o); o = align256(o + sizeof(double) * 9 * SL * (size_t)B * R);
  c.sl.f = reinterpret_cast<float*>(p + o); o = align256(o + sizeof(float) * 12 * SL * (size_t)B * R);
  c.sl.n = reinterpret_cast<int*>(p + o); o = align256(o + sizeof(int) * (size_t)B * R);
  c.sl.cnt = reinterpret_cast<int*>(p + o); o = align256(o + sizeof(int) * SL * (size_t)B * R);
  c.bytes = o + 256;
  return c;
}

template <class M>
size_t workspace_bytes(int B, int N) { return B > 0 && N > 0 ? carve<M>(nullptr, B, N).bytes : 0; }

// ------------------------------------------------------------------------------------------------------------ kernels
template <class M>
__global__ __launch_bounds__(256) void ransac_norm_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb,
                                                          const int* __restrict__ counts, const double* __restrict__ K, int N, float thr,
                                                          int max_iters, PairState<M>* __restrict__ st, float4* __restrict__ pts) {
  __shared__ double sh[256];
  const int b = blockIdx.x;
  const int n = counts ? min(max(counts[b], 0), N) : N;
  typename M::Norm nrm;
  float t2a, t2b;
  const bool valid = M::normalise(ka + (long)b * N, kb + (long)b * N, n, K ? K + (long)b * 9 : nullptr, thr, sh,
                                  pts + (long)b * N, nrm, t2a, t2b);
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
    for (int k = 0; k < 9; ++k) { S.cur[k] = 0; S.cand[k] = 0; }
    for (int k = 0; k < 12; ++k) { S.curf[k] = 0; S.candf[k] = 0; }
  }
}

// HYP_LANES lanes per (pair, hypothesis of the round), HYP_THREADS per workgroup; grid B * R * HYP_LANES / HYP_THREADS
template <class M>
__global__ __launch_bounds__(M::HYP_THREADS) void ransac_hyp_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb,
                                                                    int N, const unsigned long long* __restrict__ seeds,
                                                                    const PairState<M>* __restrict__ st, int round, Slots sl) {
  constexpr int S = M::S, L = M::HYP_LANES;
  static_assert(R % (M::HYP_THREADS / L) == 0, "a workgroup must not straddle two pairs");
  const int g = blockIdx.x * (M::HYP_THREADS / L) + threadIdx.x / L, b = g / R;
  const PairState<M>& P = st[b];
  if (P.done) return;  // uniform over the workgroup: its hypotheses belong to one pair
  const int h = round * R + g % R;
  int idx[S];
  bool act = draw_sample<S>(seeds[b], h, P.n, idx);
  double xa[S], ya[S], xb[S], yb[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const float2 a = act ? ka[(long)b * N + idx[k]] : make_float2(0.f, 0.f);
    const float2 q = act ? kb[(long)b * N + idx[k]] : make_float2(0.f, 0.f);
    act = act && finite_row(a.x, a.y, q.x, q.y);
    P.nrm.apply(a, q, xa[k], ya[k], xb[k], yb[k]);
  }
  M::hypothesis(xa, ya, xb, yb, act, g, threadIdx.x % L, sl);
}

// one wave per (pair, hypothesis): the hypothesis' models (wave-uniform coefficients) against the pair's points
template <class M>
__global__ __launch_bounds__(256) void ransac_score_kernel(const float4* __restrict__ pts, int N, const PairState<M>* __restrict__ st,
                                                           Slots sl) {
  constexpr int SL = M::SLOTS;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = g / R;
  const PairState<M>& P = st[b];
  if (P.done) return;
  const int nm = sl.n[g];
  const float* mf = sl.f + (long)g * SL * 12;
  const float4* Pp = pts + (long)b * N;
  const int n = P.n;
  const float t2a = P.thr2a, t2b = P.thr2b;
  int c[SL];
#pragma unroll
  for (int r = 0; r < SL; ++r) c[r] = 0;
  if (nm > 0) {
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const float4 p = i < n ? Pp[i] : make_float4(NAN, NAN, NAN, NAN);
#pragma unroll
      for (int r = 0; r < SL; ++r)
        if (M::SCORE_EVERY_SLOT || r < nm) c[r] += __popcll(__ballot(M::inlier(mf + 12 * r, p, t2a, t2b)));
    }
  }
  if (lane == 0) {
    int* o = sl.cnt + (long)g * SL;
#pragma unroll
    for (int r = 0; r < SL; ++r) o[r] = r < nm ? c[r] : -1;
  }
}

// one workgroup per pair: best (count, lowest slot) of the round, running best, adaptive iteration count, done flag
template <class M>
__global__ __launch_bounds__(256) void ransac_select_kernel(PairState<M>* __restrict__ st, int round, double conf, int max_iters,
                                                            Slots sl) {
  constexpr int SL = M::SLOTS;
  __shared__ int sc[256], si[256];
  const int b = blockIdx.x, t = threadIdx.x;
  PairState<M>& P = st[b];
  if (P.done) return;
  const int* cnt = sl.cnt + (long)b * R * SL;
  int bc = -1, bi = 0x7fffffff;
  for (int k = t; k < R * SL; k += 256) {
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
      P.best_h = round * R + k / SL;
      P.best_root = k % SL;
      const double* m = sl.d + ((long)b * R * SL + k) * 9;
      for (int q = 0; q < 9; ++q) P.cur[q] = m[q];
      to_f32(P.cur, P.curf);
      P.needed = update_num_iters(conf, (double)c / P.n, M::S, max_iters);
    }
    P.rounds = round + 1;
    const long drawn = (long)(round + 1) * R;
    P.done = drawn >= (long)min(max_iters, P.needed) ? 1 : 0;
  }
}

// mask[b, i] = inlier of the current model (rows beyond counts[b], and pairs without a model: 0); grid (ceil(N / 256), B)
template <class M>
__global__ __launch_bounds__(256) void ransac_mask_kernel(const float4* __restrict__ pts, int N, const PairState<M>* __restrict__ st,
                                                          unsigned char* __restrict__ mask) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const PairState<M>& P = st[b];
  bool in = false;
  if (P.best > 0 && i < P.n) in = M::inlier(P.curf, pts[(long)b * N + i], P.thr2a, P.thr2b);
  mask[(long)b * N + i] = in ? 1 : 0;
}

// one workgroup per pair: a least-squares candidate from the current mask (M::refit)
template <class M>
__global__ __launch_bounds__(256) void ransac_refit_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb, int N,
                                                           PairState<M>* __restrict__ st, const unsigned char* __restrict__ mask) {
  const long o = (long)blockIdx.x * N;
  M::refit(ka + o, kb + o, st[blockIdx.x], mask + o);
}

// one wave per pair: re-score the candidate; keep it if its count is not lower, else stop refining
template <class M>
__global__ __launch_bounds__(64) void ransac_accept_kernel(const float4* __restrict__ pts, int N, PairState<M>* __restrict__ st) {
  const int b = blockIdx.x, lane = threadIdx.x;
  PairState<M>& P = st[b];
  if (P.stop || !P.cand_ok) return;
  const float4* Pp = pts + (long)b * N;
  const int n = P.n;
  const float t2a = P.thr2a, t2b = P.thr2b;
  int c = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const float4 p = i < n ? Pp[i] : make_float4(NAN, NAN, NAN, NAN);
    c += __popcll(__ballot(M::inlier(P.candf, p, t2a, t2b)));
  }
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

// one thread per pair: ok flag, M::finish (model, info row)
template <class M>
__global__ __launch_bounds__(64) void ransac_finish_kernel(int B, const PairState<M>* __restrict__ st, double* __restrict__ out,
                                                           unsigned char* __restrict__ ok, int* __restrict__ info) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const PairState<M>& P = st[b];
  const bool good = P.valid && P.best > 0;
  M::finish(P, good, out + (long)b * 9, info + (long)b * M::INFO);
  ok[b] = good ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ host
// the argument checks of every RANSAC entry point: `op` prefixes each message, `conf` names the confidence argument
int check_args(const char* op, const char* conf, bool pointers, int B, int N, float threshold, double confidence, int max_iters,
               size_t ws_bytes, size_t ws_need) {
  const std::string o(op);
  ROMA_REQUIRE(pointers, o + ": null pointer");
  ROMA_REQUIRE(B > 0 && N > 0 && (long)B * N < (1l << 31) && B <= (1 << 16), o + ": need 0 < B <= 65536, 0 < N, B * N < 2^31");
  ROMA_REQUIRE(max_iters > 0, o + ": max_iters must be positive");
  ROMA_REQUIRE(threshold > 0 && isfinite(threshold), o + ": threshold must be positive and finite");
  ROMA_REQUIRE(confidence >= 0 && confidence <= 1, o + ": " + conf + " must lie in [0, 1]");
  ROMA_REQUIRE(ws_bytes >= ws_need, o + ": workspace too small (roma_op_" + o + "_workspace)");
  return 0;
}

// the launch sequence of the pipeline above; K: [B, 3, 3] f64 camera matrices or NULL, read by M::normalise only
template <class M>
int ransac_run(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, const double* K, int B,
               int N, float thr, double conf, int max_iters, bool refine, double* out_model, unsigned char* out_mask,
               unsigned char* out_ok, int* out_info, void* ws, hipStream_t s) {
  const Carve<M> c = carve<M>(align_base<void*>(ws), B, N);
  const float2* ka = reinterpret_cast<const float2*>(kpts_a);
  const float2* kb = reinterpret_cast<const float2*>(kpts_b);
  hipLaunchKernelGGL(ransac_norm_kernel<M>, dim3(B), dim3(256), 0, s, ka, kb, counts, K, N, thr, max_iters, c.st, c.pts);
  ROMA_LAUNCH_CHECK();
  const int rounds = (max_iters + R - 1) / R;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(ransac_hyp_kernel<M>, dim3(B * R * M::HYP_LANES / M::HYP_THREADS), dim3(M::HYP_THREADS), 0, s, ka, kb, N,
                       seeds, c.st, r, c.sl);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_score_kernel<M>, dim3(B * R / 4), dim3(256), 0, s, c.pts, N, c.st, c.sl);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_select_kernel<M>, dim3(B), dim3(256), 0, s, c.st, r, conf, max_iters, c.sl);
    ROMA_LAUNCH_CHECK();
  }
  const dim3 mgrid((N + 255) / 256, B);
  if constexpr (M::REFINE_ITERS > 0) {
    for (int it = 0; refine && it < M::REFINE_ITERS; ++it) {
      hipLaunchKernelGGL(ransac_mask_kernel<M>, mgrid, dim3(256), 0, s, c.pts, N, c.st, out_mask);
      ROMA_LAUNCH_CHECK();
      hipLaunchKernelGGL(ransac_refit_kernel<M>, dim3(B), dim3(256), 0, s, ka, kb, N, c.st, out_mask);
      ROMA_LAUNCH_CHECK();
      hipLaunchKernelGGL(ransac_accept_kernel<M>, dim3(B), dim3(64), 0, s, c.pts, N, c.st);
      ROMA_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(ransac_mask_kernel<M>, mgrid, dim3(256), 0, s, c.pts, N, c.st, out_mask);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(ransac_finish_kernel<M>, dim3((B + 63) / 64), dim3(64), 0, s, B, c.st, out_model, out_ok, out_info);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ MAGSAC++
// The same pipeline with MAGSAC++ scoring (Barath et al., CVPR 2020; nu = 4; tools/magsac_ref.py restates it): a model's score
// is the sum over the pair's rows of the loss rho(V), V = r^2 k^2 / (2 tau^2) with r the model's pixel residual (M::residual2)
// and tau the threshold (M::mag_thr2: both in the model's own units - pixels for H and F, normalised camera coordinates for E);
// lower is better.  Sampling rounds, hypotheses and slots are those above (ransac_norm_kernel and ransac_hyp_kernel are shared);
// what changes:
//   magsac_score_kernel  one wave per hypothesis: compensated f32 sum of rho per slot (lane partials over rows i = lane mod 64
//                        ascending, then a fixed butterfly), and the count r < tau for the adaptive iteration count
//   magsac_select_kernel arg-min (ties: lowest (h, slot)); the running best changes only on a strictly smaller score
//   lo_iters times magsac_refit_kernel (M::wrefit: IRLS step, weights w(V) of the current model) and magsac_accept_kernel (the
//   candidate is kept only if its score is strictly lower - the gain measured paired, on the same rows - else LO stops); then
//   the mask r < tau and magsac_finish_kernel (M::mag_finish: the model and the first M::MAG_INFO - 1 entries of the info row).
// From the policy it needs residual2 / res_terms / r2_from / NT, res_scales, mag_thr2, wrefit, mag_finish, MAG_INFO.
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
  double gain;                  // what the accepted LO steps lowered the sum of rho by (magsac_accept_kernel)
};

template <class M>
struct MagCarve {
  Carve<M> c;                   // the RANSAC carve: pair states, points, slots (cnt: inlier counts per slot)
  MagState* ms;
  float* sc;                    // sum of rho per slot, +inf if unused [B * R * SLOTS]
  size_t bytes;
};

template <class M>
MagCarve<M> magsac_carve(void* ws, int B, int N) {
  MagCarve<M> m;
  m.c = carve<M>(ws, B, N);
  char* p = static_cast<char*>(ws);
  size_t o = m.c.bytes - 256;
  m.ms = reinterpret_cast<MagState*>(p + o); o = align256(o + sizeof(MagState) * B);
  m.sc = reinterpret_cast<float*>(p + o); o = align256(o + sizeof(float) * M::SLOTS * (size_t)B * R);
  m.bytes = o + 256;
  return m;
}

template <class M>
size_t magsac_workspace_bytes(int B, int N) { return B > 0 && N > 0 ? magsac_carve<M>(nullptr, B, N).bytes : 0; }

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

// one thread per pair: residual scales, V scale, threshold (M::mag_thr2: tau^2 in the units of M::residual2)
template <class M>
__global__ __launch_bounds__(64) void magsac_init_kernel(int B, float thr, const PairState<M>* __restrict__ st,
                                                         MagState* __restrict__ ms) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  MagState& S = ms[b];
  M::res_scales(st[b].nrm, S.sa2, S.sb2);
  const double t2 = M::mag_thr2(st[b].nrm, thr);
  S.vs = (float)(MAGSAC_K2 / (2 * t2));
  S.t2 = (float)t2;
  S.score = INFINITY;
  S.score_min = INFINITY;
  S.lo_steps = 0;
  S.gain = 0.0;
}

// one wave per (pair, hypothesis)
template <class M>
__global__ __launch_bounds__(256) void magsac_score_kernel(const float4* __restrict__ pts, int N, const PairState<M>* __restrict__ st,
                                                           const MagState* __restrict__ ms, Slots sl, float* __restrict__ sc) {
  constexpr int SL = M::SLOTS;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = g / R;
  const PairState<M>& P = st[b];
  if (P.done) return;
  const int nm = sl.n[g];
  float acc[SL];
  int c[SL];
#pragma unroll
  for (int r = 0; r < SL; ++r) { acc[r] = 0.f; c[r] = 0; }
  if (nm > 0) magsac_sums<M, SL>(sl.f + (long)g * SL * 12, nm, pts + (long)b * N, P.n, ms[b], lane, acc, c);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < SL; ++r) {
      sc[(long)g * SL + r] = r < nm ? acc[r] : INFINITY;
      sl.cnt[(long)g * SL + r] = r < nm ? c[r] : -1;
    }
  }
}

// one workgroup per pair: smallest score of the round (lowest slot on ties), running best, adaptive iteration count, done flag
template <class M>
__global__ __launch_bounds__(256) void magsac_select_kernel(PairState<M>* __restrict__ st, MagState* __restrict__ ms, int round,
                                                            double conf, int max_iters, Slots sl, const float* __restrict__ sc) {
  constexpr int SL = M::SLOTS;
  __shared__ float ss[256];
  __shared__ int si[256];
  const int b = blockIdx.x, t = threadIdx.x;
  PairState<M>& P = st[b];
  if (P.done) return;
  const float* s = sc + (long)b * R * SL;
  float bs = INFINITY;
  int bi = 0x7fffffff;
  for (int k = t; k < R * SL; k += 256) {
    const float v = s[k];
    if (v < bs) { bs = v; bi = k; }  // k ascends: ties keep the lower slot
  }
  ss[t] = bs;
  si[t] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const float v = ss[t + w];
      const int i = si[t + w];
      if (v < ss[t] || (v == ss[t] && i < si[t])) { ss[t] = v; si[t] = i; }
    }
    __syncthreads();
  }
  if (t == 0) {
    MagState& S = ms[b];
    const float v = ss[0];
    const int k = si[0];
    if (v < S.score) {  // strictly: an earlier round's model keeps a tie
      S.score = v;
      S.score_min = v;
      const int c = sl.cnt[(long)b * R * SL + k];
      P.best = c;
      P.best_min = c;
      P.best_h = round * R + k / SL;
      P.best_root = k % SL;
      const double* m = sl.d + ((long)b * R * SL + k) * 9;
      for (int q = 0; q < 9; ++q) P.cur[q] = m[q];
      to_f32(P.cur, P.curf);
      P.needed = update_num_iters(conf, (double)c / P.n, M::S, max_iters);
    }
    P.rounds = round + 1;
    const long drawn = (long)(round + 1) * R;
    P.done = drawn >= (long)min(max_iters, P.needed) ? 1 : 0;
  }
}

// one workgroup per pair: an IRLS candidate from the MAGSAC++ weights of the current model (M::wrefit)
template <class M>
__global__ __launch_bounds__(256) void magsac_refit_kernel(const float2* __restrict__ ka, const float2* __restrict__ kb,
                                                           const float4* __restrict__ pts, int N, PairState<M>* __restrict__ st,
                                                           const MagState* __restrict__ ms) {
  const long o = (long)blockIdx.x * N;
  M::wrefit(ka + o, kb + o, pts + o, st[blockIdx.x], ms[blockIdx.x]);
}

// one wave per pair: keep the candidate if its sum of rho is strictly lower than the current model's, else stop.  The gain
// sum(rho_cur - rho_cand) is measured on the same rows in one pass, the candidate's residual terms as the current model's
// plus those of the f32 difference (cand - cur): rounding the two models to f32 separately moves each sum by far more than a
// late IRLS step gains (an inlier's residual is a small difference of O(1) normalised terms), and paired this way the shared
// part of that error cancels.  The inlier count is the candidate's own (what the mask kernel evaluates).
template <class M>
__global__ __launch_bounds__(64) void magsac_accept_kernel(const float4* __restrict__ pts, int N, PairState<M>* __restrict__ st,
                                                           MagState* __restrict__ ms) {
  constexpr int NT = M::NT;
  const int b = blockIdx.x, lane = threadIdx.x;
  PairState<M>& P = st[b];
  if (P.stop || !P.cand_ok) return;
  MagState& S = ms[b];
  float dm[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) dm[k] = (float)(P.cand[k] - P.cur[k]);
  const float4* Pp = pts + (long)b * N;
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
    float w;
    const float ru = magsac_rho(M::r2_from(tu, sa2, sb2) * vs, w);
    const float rc = magsac_rho(M::r2_from(tc, sa2, sb2) * vs, w);
    two_sum(g, gc, row ? ru - rc : 0.f);
    c += __popcll(__ballot(M::residual2(P.candf, p, sa2, sb2) < t2));
  }
  g = wave_total(g, gc);
  if (lane == 0) {
    if (g > 0.f) {
      S.gain = S.gain + (double)g;
      S.lo_steps = S.lo_steps + 1;
      P.best = c;
      for (int k = 0; k < 9; ++k) P.cur[k] = P.cand[k];
      for (int k = 0; k < 12; ++k) P.curf[k] = P.candf[k];
    } else {
      P.stop = 1;
    }
    P.cand_ok = 0;
  }
}

// mask[b, i] = r < tau under the current model (rows beyond counts[b], and pairs without inliers: 0); grid (ceil(N / 256), B)
template <class M>
__global__ __launch_bounds__(256) void magsac_mask_kernel(const float4* __restrict__ pts, int N, const PairState<M>* __restrict__ st,
                                                          const MagState* __restrict__ ms, unsigned char* __restrict__ mask) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const PairState<M>& P = st[b];
  bool in = false;
  if (P.best > 0 && i < P.n) {
    const MagState& S = ms[b];
    in = M::residual2(P.curf, pts[(long)b * N + i], S.sa2, S.sb2) < S.t2;
  }
  mask[(long)b * N + i] = in ? 1 : 0;
}

// one thread per pair: ok flag, M::mag_finish (model, the first M::MAG_INFO - 1 entries of the info row), LO steps, scores (the final sum
// of rho is the winning minimal model's less the gains of the accepted LO steps)
template <class M>
__global__ __launch_bounds__(64) void magsac_finish_kernel(int B, const PairState<M>* __restrict__ st, const MagState* __restrict__ ms,
                                                           double* __restrict__ out, unsigned char* __restrict__ ok,
                                                           int* __restrict__ info, double* __restrict__ score) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const PairState<M>& P = st[b];
  const MagState& S = ms[b];
  const bool good = P.valid && P.best > 0;
  M::mag_finish(P, good, out + (long)b * 9, info + (long)b * M::MAG_INFO);
  info[(long)b * M::MAG_INFO + M::MAG_INFO - 1] = S.lo_steps;
  const bool found = P.best_h >= 0;
  score[2 * (long)b] = found ? (double)S.score_min : 0.0;
  score[2 * (long)b + 1] = found ? (double)S.score_min - S.gain : 0.0;
  ok[b] = good ? 1 : 0;
}

template <class M>
int magsac_run(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, const double* K, int B,
               int N, float thr,
               double conf, int max_iters, int lo_iters, double* out_model, unsigned char* out_mask, unsigned char* out_ok,
               int* out_info, double* out_score, void* ws, hipStream_t s) {
  const MagCarve<M> w = magsac_carve<M>(align_base<void*>(ws), B, N);
  const Carve<M>& c = w.c;
  const float2* ka = reinterpret_cast<const float2*>(kpts_a);
  const float2* kb = reinterpret_cast<const float2*>(kpts_b);
  hipLaunchKernelGGL(ransac_norm_kernel<M>, dim3(B), dim3(256), 0, s, ka, kb, counts, K, N, thr, max_iters, c.st, c.pts);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(magsac_init_kernel<M>, dim3((B + 63) / 64), dim3(64), 0, s, B, thr, c.st, w.ms);
  ROMA_LAUNCH_CHECK();
  const int rounds = (max_iters + R - 1) / R;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(ransac_hyp_kernel<M>, dim3(B * R * M::HYP_LANES / M::HYP_THREADS), dim3(M::HYP_THREADS), 0, s, ka, kb, N,
                       seeds, c.st, r, c.sl);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(magsac_score_kernel<M>, dim3(B * R / 4), dim3(256), 0, s, c.pts, N, c.st, w.ms, c.sl, w.sc);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(magsac_select_kernel<M>, dim3(B), dim3(256), 0, s, c.st, w.ms, r, conf, max_iters, c.sl, w.sc);
    ROMA_LAUNCH_CHECK();
  }
  for (int it = 0; it < lo_iters; ++it) {
    hipLaunchKernelGGL(magsac_refit_kernel<M>, dim3(B), dim3(256), 0, s, ka, kb, c.pts, N, c.st, w.ms);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(magsac_accept_kernel<M>, dim3(B), dim3(64), 0, s, c.pts, N, c.st, w.ms);
    ROMA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(magsac_mask_kernel<M>, dim3((N + 255) / 256, B), dim3(256), 0, s, c.pts, N, c.st, w.ms, out_mask);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(magsac_finish_kernel<M>, dim3((B + 63) / 64), dim3(64), 0, s, B, c.st, w.ms, out_model, out_ok, out_info,
                     out_score);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace roma
