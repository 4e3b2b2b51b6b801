// Ground-truth warp from sensor depth (roma_op_warp_kpts: the reference's warp_kpts and get_gt_warp, romatch/utils/utils.py) and
// the dense EPE / PCK metrics of a warp against it (roma_op_dense_metrics: MegadepthDenseBenchmark.geometric_dist).  The definition
// is stated in include/roma_hip.h and restated, operation by operation, in numpy float64 by tools/gt_warp_ref.py - the oracle of
// tests/test_gpu_gt_warp.py.
//
// Three kernels:
//   1. warp_kpts_kernel             one key point per thread: sample depth0, unproject, move, project, sample depth1, compare.  The
//                                   key points are read (f32 or f64) or generated (the pixel centres of a grid_h x grid_w grid);
//   2. dense_metrics_kernel         the same chain on columns 0:2 of a warp, then the pixel distance of columns 2:4 to the result,
//                                   summed per thread (ascending index), per wave (shuffle tree), per workgroup (wave order);
//   3. dense_metrics_finish_kernel  the per-workgroup partials summed in index order per pair, the batch means in pair order.
// Grids are (blocks, pair) with the blocks of a pair capped at a number that does not depend on B and a block-stride loop, so the
// partition of a pair's pixels - and with it every per-pair bit - is independent of B and of where the pair sits in the batch.
// The 30 doubles of a pair (K0^-1, R, t, K1) are formed by thread 0 of each workgroup and read from LDS into vector registers:
// the float64 chain has more wave-uniform values than a wave has scalar registers (as triangulate_kernel had).  No float is added
// atomically, nothing is read back.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "common.h"

// nothing here is fused: tools/gt_warp_ref.py evaluates the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int GW_THREADS = 256;
constexpr int GW_WAVES = GW_THREADS / 64;
constexpr int GW_PAIR_BLOCKS = 256;  // blocks of one pair at most: independent of B, the rest is the block-stride loop
constexpr int GW_MAX_SIDE = 32768;
constexpr int GW_PAIR_DOUBLES = 30;  // K0^-1 [9], R [9], t [3], K1 [9]

struct Pair {
  double ki[9], r[9], t[3], k1[9];
};

struct Sizes {
  int H0, W0, H1, W1;
};

// thread 0: the pair's matrices into LDS.  K0^-1 = adjugate / determinant of a general 3 x 3, in this order.
__device__ __forceinline__ void load_pair(double* s, const double* T, int t_rows, const double* K0, const double* K1, int b) {
  const double* k = K0 + (long)b * 9;
  const double a = k[0], bb = k[1], c = k[2], d = k[3], e = k[4], f = k[5], g = k[6], h = k[7], i = k[8];
  const double c00 = e * i - f * h, c01 = c * h - bb * i, c02 = bb * f - c * e;
  const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
  const double c20 = d * h - e * g, c21 = bb * g - a * h, c22 = a * e - bb * d;
  const double det = (a * c00 + bb * c10) + c * c20;
  s[0] = c00 / det, s[1] = c01 / det, s[2] = c02 / det;
  s[3] = c10 / det, s[4] = c11 / det, s[5] = c12 / det;
  s[6] = c20 / det, s[7] = c21 / det, s[8] = c22 / det;
  const double* t = T + (long)b * t_rows * 4;
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) s[9 + r * 3 + q] = t[r * 4 + q];
    s[18 + r] = t[r * 4 + 3];
  }
  const double* k1 = K1 + (long)b * 9;
  for (int q = 0; q < 9; ++q) s[21 + q] = k1[q];
}

__device__ __forceinline__ Pair read_pair(const double* s) {
  Pair p;
#pragma unroll
  for (int q = 0; q < 9; ++q) p.ki[q] = s[q], p.r[q] = s[9 + q], p.k1[q] = s[21 + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) p.t[q] = s[18 + q];
  return p;
}

// torch grid_sample, bilinear, align_corners=False, zeros padding, of one f32 map in float64.  In and out of range is decided in
// float64 (every comparison with NaN is false) before anything becomes an integer; a tap that is out of range forms no address
// and contributes 0.
__device__ __forceinline__ double sample(const float* D, int Hs, int Ws, double x, double y) {
  const double ix = ((x + 1.0) * (double)Ws - 1.0) / 2.0, iy = ((y + 1.0) * (double)Hs - 1.0) / 2.0;
  const double x0 = floor(ix), y0 = floor(iy);
  const double x1 = x0 + 1.0, y1 = y0 + 1.0;
  const double wx0 = x1 - ix, wx1 = ix - x0, wy0 = y1 - iy, wy1 = iy - y0;
  const double xm = (double)(Ws - 1), ym = (double)(Hs - 1);
  const bool w_in = x0 >= 0.0 && x0 <= xm, e_in = x1 >= 0.0 && x1 <= xm;
  const bool n_in = y0 >= 0.0 && y0 <= ym, s_in = y1 >= 0.0 && y1 <= ym;
  // where a column or row is out of range its index is not used; -1 <= x0 <= Ws - 1 where either column is in range
  const int xi = (w_in || e_in) ? (int)x0 : 0, yi = (n_in || s_in) ? (int)y0 : 0;
  const long row_n = (long)yi * Ws, row_s = row_n + Ws;
  double acc = (n_in && w_in) ? (double)D[row_n + xi] * (wx0 * wy0) : 0.0;
  acc = acc + ((n_in && e_in) ? (double)D[row_n + xi + 1] * (wx1 * wy0) : 0.0);
  acc = acc + ((s_in && w_in) ? (double)D[row_s + xi] * (wx0 * wy1) : 0.0);
  acc = acc + ((s_in && e_in) ? (double)D[row_s + xi + 1] * (wx1 * wy1) : 0.0);
  return acc;
}

struct Warped {
  double wx, wy, rel;
  bool valid;
};

// one key point (x, y) normalised in image 0
__device__ __forceinline__ Warped warp_point(const Pair& P, const float* depth0, const float* depth1, const Sizes& S, double thr, double x,
                                             double y) {
  const double px = (double)S.W0 * (x + 1.0) / 2.0, py = (double)S.H0 * (y + 1.0) / 2.0;
  const double d0 = sample(depth0, S.H0, S.W0, x, y);
  const bool nonzero = d0 != 0.0;
  const double h0 = px * d0, h1 = py * d0, h2 = d0;
  const double X0 = (P.ki[0] * h0 + P.ki[1] * h1) + P.ki[2] * h2;
  const double X1 = (P.ki[3] * h0 + P.ki[4] * h1) + P.ki[5] * h2;
  const double X2 = (P.ki[6] * h0 + P.ki[7] * h1) + P.ki[8] * h2;
  const double Y0 = ((P.r[0] * X0 + P.r[1] * X1) + P.r[2] * X2) + P.t[0];
  const double Y1 = ((P.r[3] * X0 + P.r[4] * X1) + P.r[5] * X2) + P.t[1];
  const double Y2 = ((P.r[6] * X0 + P.r[7] * X1) + P.r[8] * X2) + P.t[2];
  const double P0 = (P.k1[0] * Y0 + P.k1[1] * Y1) + P.k1[2] * Y2;
  const double P1 = (P.k1[3] * Y0 + P.k1[4] * Y1) + P.k1[5] * Y2;
  const double P2 = (P.k1[6] * Y0 + P.k1[7] * Y1) + P.k1[8] * Y2;
  const double den = P2 + 1e-4;
  const double u = P0 / den, v = P1 / den;
  const bool covisible = u > 0.0 && u < (double)(S.W1 - 1) && v > 0.0 && v < (double)(S.H1 - 1);
  Warped o;
  o.wx = 2.0 * u / (double)S.W1 - 1.0, o.wy = 2.0 * v / (double)S.H1 - 1.0;
  const double d1 = sample(depth1, S.H1, S.W1, o.wx, o.wy);
  o.rel = fabs((d1 - Y2) / d1);
  o.valid = nonzero && covisible && o.rel < thr;
  return o;
}

// value j of the n pixel centres of [-1, 1]: (2 j + 1) / n - 1 in float64, rounded once to float32 (what a matcher stores)
__device__ __forceinline__ double grid_value(int j, int n) { return (double)(float)((2.0 * (double)j + 1.0) / (double)n - 1.0); }

struct WarpParams {
  const void* kpts;
  int kpts_f64, grid_h, grid_w;
  const float* depth0;
  const float* depth1;
  const double* T;
  int t_rows;
  const double* K0;
  const double* K1;
  long L;
  Sizes S;
  double thr;
  unsigned char* valid;
  float* prob;
  double* rel;
  double* warped;
};

// grid (blocks, B)
__global__ __launch_bounds__(GW_THREADS) void warp_kpts_kernel(const WarpParams A) {
  __shared__ double s_pair[GW_PAIR_DOUBLES];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) load_pair(s_pair, A.T, A.t_rows, A.K0, A.K1, b);
  __syncthreads();
  const Pair P = read_pair(s_pair);
  const float* depth0 = A.depth0 + (long)b * A.S.H0 * A.S.W0;
  const float* depth1 = A.depth1 + (long)b * A.S.H1 * A.S.W1;
  const long base = (long)b * A.L;
  const long stride = (long)gridDim.x * GW_THREADS;
  for (long k = (long)blockIdx.x * GW_THREADS + threadIdx.x; k < A.L; k += stride) {
    double x, y;
    if (!A.kpts) {
      const int row = (int)(k / A.grid_w);
      x = grid_value((int)(k - (long)row * A.grid_w), A.grid_w), y = grid_value(row, A.grid_h);
    } else if (A.kpts_f64) {
      const double* p = static_cast<const double*>(A.kpts) + (base + k) * 2;
      x = p[0], y = p[1];
    } else {
      const float* p = static_cast<const float*>(A.kpts) + (base + k) * 2;
      x = (double)p[0], y = (double)p[1];
    }
    const Warped o = warp_point(P, depth0, depth1, A.S, A.thr, x, y);
    A.warped[(base + k) * 2] = o.wx, A.warped[(base + k) * 2 + 1] = o.wy;
    if (A.valid) A.valid[base + k] = o.valid ? 1 : 0;
    if (A.prob) A.prob[base + k] = o.valid ? 1.0f : 0.0f;
    if (A.rel) A.rel[base + k] = o.rel;
  }
}

struct MetricParams {
  const float* matches;
  long batch_stride, row_stride;  // floats
  const float* depth1;
  const float* depth2;
  const double* T;
  int t_rows;
  const double* K1;
  const double* K2;
  int h, w;
  Sizes S;
  double thr, pck0, pck1, pck2;
  float* prob;
  double* gd;
  double* part_sum;     // [B, blocks]
  long long* part_cnt;  // [B, blocks, 4]: valid, below pck0, pck1, pck2
};

// grid (blocks, B) over the h x w pixels of a pair
__global__ __launch_bounds__(GW_THREADS) void dense_metrics_kernel(const MetricParams A) {
  __shared__ double s_pair[GW_PAIR_DOUBLES];
  __shared__ double s_sum[GW_WAVES];
  __shared__ int s_cnt[GW_WAVES][4];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) load_pair(s_pair, A.T, A.t_rows, A.K1, A.K2, b);
  __syncthreads();
  const Pair P = read_pair(s_pair);
  const float* depth1 = A.depth1 + (long)b * A.S.H0 * A.S.W0;
  const float* depth2 = A.depth2 + (long)b * A.S.H1 * A.S.W1;
  const float* m = A.matches + (long)b * A.batch_stride;
  const long n = (long)A.h * A.w, base = (long)b * n;
  const float wf = (float)A.w, hf = (float)A.h;
  const double nan_ = __longlong_as_double(0x7ff8000000000000ll);
  double sum = 0.0;
  int cnt[4] = {0, 0, 0, 0};
  const long stride = (long)gridDim.x * GW_THREADS;
  for (long k = (long)blockIdx.x * GW_THREADS + threadIdx.x; k < n; k += stride) {
    const int row = (int)(k / A.w), col = (int)(k - (long)row * A.w);
    const f32x4 q = *reinterpret_cast<const f32x4*>(m + (long)row * A.row_stride + 4l * col);
    const Warped o = warp_point(P, depth1, depth2, A.S, A.thr, (double)q[0], (double)q[1]);
    // the prediction in pixels of the warp grid, in float32 as the reference forms it; the truth in float64
    const float xh = (wf * (q[2] + 1.0f)) / 2.0f, yh = (hf * (q[3] + 1.0f)) / 2.0f;
    const double tx = (double)A.w * (o.wx + 1.0) / 2.0, ty = (double)A.h * (o.wy + 1.0) / 2.0;
    const double dx = (double)xh - tx, dy = (double)yh - ty;
    const double gd = sqrt(dx * dx + dy * dy);
    if (o.valid) {
      sum = sum + gd;
      cnt[0] += 1, cnt[1] += gd < A.pck0 ? 1 : 0, cnt[2] += gd < A.pck1 ? 1 : 0, cnt[3] += gd < A.pck2 ? 1 : 0;
    }
    if (A.prob) A.prob[base + k] = o.valid ? 1.0f : 0.0f;
    if (A.gd) A.gd[base + k] = o.valid ? gd : nan_;
  }
  // fixed tree over the wave, then the waves in order
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sum = sum + __shfl_down(sum, off);
#pragma unroll
    for (int c = 0; c < 4; ++c) cnt[c] += __shfl_down(cnt[c], off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_sum[wave] = sum;
#pragma unroll
    for (int c = 0; c < 4; ++c) s_cnt[wave][c] = cnt[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s_sum[0];
    int c4[4] = {s_cnt[0][0], s_cnt[0][1], s_cnt[0][2], s_cnt[0][3]};
    for (int v = 1; v < GW_WAVES; ++v) {
      t = t + s_sum[v];
      for (int c = 0; c < 4; ++c) c4[c] += s_cnt[v][c];
    }
    const long slot = (long)b * gridDim.x + blockIdx.x;
    A.part_sum[slot] = t;
    for (int c = 0; c < 4; ++c) A.part_cnt[slot * 4 + c] = (long long)c4[c];
  }
}

struct FinishParams {
  const double* part_sum;
  const long long* part_cnt;
  int B, blocks;
  long long* n_valid;
  long long* n_below;
  double* gd_sum;
  double* epe;
  double* pck;
};

// one workgroup: a thread per pair sums its partials in index order; thread 0 then sums the pairs in pair order
__global__ __launch_bounds__(GW_THREADS) void dense_metrics_finish_kernel(const FinishParams A) {
  for (int b = threadIdx.x; b < A.B; b += GW_THREADS) {
    double t = 0.0;
    long long c4[4] = {0, 0, 0, 0};
    for (int i = 0; i < A.blocks; ++i) {
      const long slot = (long)b * A.blocks + i;
      t = t + A.part_sum[slot];
      for (int c = 0; c < 4; ++c) c4[c] += A.part_cnt[slot * 4 + c];
    }
    A.gd_sum[b] = t, A.n_valid[b] = c4[0];
    for (int c = 0; c < 3; ++c) A.n_below[(long)b * 3 + c] = c4[1 + c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    long long c4[4] = {0, 0, 0, 0};
    for (int b = 0; b < A.B; ++b) {
      t = t + A.gd_sum[b];
      c4[0] += A.n_valid[b];
      for (int c = 0; c < 3; ++c) c4[1 + c] += A.n_below[(long)b * 3 + c];
    }
    // no valid pixel: 0 / 0 = NaN, the mean of an empty selection
    const double nv = (double)c4[0];
    A.epe[0] = t / nv;
    for (int c = 0; c < 3; ++c) A.pck[c] = (double)c4[1 + c] / nv;
  }
}

unsigned pair_blocks(long n) { return (unsigned)std::max<long>(1, std::min<long>((n + GW_THREADS - 1) / GW_THREADS, GW_PAIR_BLOCKS)); }

bool side_ok(int v) { return v >= 1 && v <= GW_MAX_SIDE; }

}  // namespace

extern "C" int roma_op_warp_kpts(const void* kpts, int kpts_f64, int grid_h, int grid_w, const float* depth0, const float* depth1,
                                 const double* T, int t_rows, const double* K0, const double* K1, int B, long L, int H0, int W0, int H1,
                                 int W1, double rel_thresh, unsigned char* valid, float* prob, double* rel, double* warped, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(depth0 && depth1 && T && K0 && K1 && warped, "warp_kpts: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "warp_kpts: B must lie in [0, 65535]");
  ROMA_REQUIRE(L >= 0, "warp_kpts: L must not be negative");
  ROMA_REQUIRE(B == 0 || L < (1l << 31) / B + ((1l << 31) % B != 0), "warp_kpts: B * L must be below 2^31");
  ROMA_REQUIRE(t_rows == 3 || t_rows == 4, "warp_kpts: t_rows must be 3 ([B, 3, 4]) or 4 ([B, 4, 4])");
  ROMA_REQUIRE(kpts_f64 == 0 || kpts_f64 == 1, "warp_kpts: kpts_f64 must be 0 (float32) or 1 (float64)");
  ROMA_REQUIRE(side_ok(H0) && side_ok(W0) && side_ok(H1) && side_ok(W1), "warp_kpts: depth sizes must lie in [1, 32768]");
  ROMA_REQUIRE(kpts || (side_ok(grid_h) && side_ok(grid_w) && (long)grid_h * grid_w == L),
               "warp_kpts: without kpts the grid must lie in [1, 32768]^2 with grid_h * grid_w = L");
  ROMA_REQUIRE(!kpts || (reinterpret_cast<uintptr_t>(kpts) & (kpts_f64 ? 7 : 3)) == 0, "warp_kpts: kpts is not aligned to its type");
  ROMA_REQUIRE(rel_thresh >= 0, "warp_kpts: the relative depth error threshold is negative (or NaN)");
  if (B == 0 || L == 0) return 0;
  WarpParams A = {kpts, kpts_f64, grid_h, grid_w, depth0, depth1, T, t_rows, K0, K1, L, {H0, W0, H1, W1}, rel_thresh, valid, prob, rel,
                  warped};
  ProfScope ps("warp_kpts_kernel", (double)B * (double)L * 56.0, "B", s);
  hipLaunchKernelGGL(warp_kpts_kernel, dim3(pair_blocks(L), B), dim3(GW_THREADS), 0, s, A);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" long roma_op_dense_metrics_workspace(int B, int h, int w) {
  if (B < 0 || B > 65535 || h < 0 || w < 0 || h > GW_MAX_SIDE || w > GW_MAX_SIDE) return -1;
  return std::max<long>(16, (long)B * pair_blocks((long)h * w) * 5 * (long)sizeof(double));
}

extern "C" int roma_op_dense_metrics(const float* matches, long batch_stride, long row_stride, const float* depth1, const float* depth2,
                                     const double* T, int t_rows, const double* K1, const double* K2, int B, int h, int w, int H1, int W1,
                                     int H2, int W2, double rel_thresh, double thr0, double thr1, double thr2, long long* n_valid,
                                     long long* n_below, double* gd_sum, double* epe, double* pck, float* prob, double* gd, void* workspace,
                                     long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(matches && depth1 && depth2 && T && K1 && K2 && n_valid && n_below && gd_sum && epe && pck && workspace,
               "dense_metrics: null pointer");
  ROMA_REQUIRE(B >= 1 && B <= 65535, "dense_metrics: B must lie in [1, 65535]");
  ROMA_REQUIRE(side_ok(h) && side_ok(w), "dense_metrics: the warp grid (h, w) must lie in [1, 32768]^2");
  ROMA_REQUIRE((long)h * w < (1l << 31) / B + ((1l << 31) % B != 0), "dense_metrics: B * h * w must be below 2^31");
  ROMA_REQUIRE(t_rows == 3 || t_rows == 4, "dense_metrics: t_rows must be 3 ([B, 3, 4]) or 4 ([B, 4, 4])");
  ROMA_REQUIRE(side_ok(H1) && side_ok(W1) && side_ok(H2) && side_ok(W2), "dense_metrics: depth sizes must lie in [1, 32768]");
  ROMA_REQUIRE(row_stride >= 4l * w && row_stride % 4 == 0 && batch_stride >= (long)(h - 1) * row_stride + 4l * w && batch_stride % 4 == 0,
               "dense_metrics: strides (in floats) must be multiples of 4 with row_stride >= 4 w and batch_stride >= (h - 1) row_stride + 4 w");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(matches) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "dense_metrics: matches must be 16-byte and workspace 8-byte aligned");
  ROMA_REQUIRE(rel_thresh >= 0 && thr0 >= 0 && thr1 >= 0 && thr2 >= 0, "dense_metrics: a threshold is negative (or NaN)");
  ROMA_REQUIRE(workspace_bytes >= roma_op_dense_metrics_workspace(B, h, w), "dense_metrics: workspace is too small");
  const unsigned blocks = pair_blocks((long)h * w);
  double* part_sum = static_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(part_sum + (long)B * blocks);
  MetricParams A = {matches, batch_stride, row_stride, depth1, depth2, T, t_rows, K1, K2, h, w, {H1, W1, H2, W2}, rel_thresh, thr0, thr1,
                    thr2, prob, gd, part_sum, part_cnt};
  {
    ProfScope ps("dense_metrics_kernel", (double)B * (double)h * (double)w * 48.0, "B", s);
    hipLaunchKernelGGL(dense_metrics_kernel, dim3(blocks, B), dim3(GW_THREADS), 0, s, A);
    ROMA_LAUNCH_CHECK();
  }
  FinishParams F = {part_sum, part_cnt, B, (int)blocks, n_valid, n_below, gd_sum, epe, pck};
  {
    ProfScope ps("dense_metrics_finish_kernel", (double)B * blocks * 40.0, "B", s);
    hipLaunchKernelGGL(dense_metrics_finish_kernel, dim3(1), dim3(GW_THREADS), 0, s, F);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace roma
