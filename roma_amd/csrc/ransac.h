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

}  // namespace
}  // namespace roma
