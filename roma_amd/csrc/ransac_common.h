// Device helpers shared by the RANSAC sources (geometry.hip: H and F; essential.hip: E): the counter-based sample stream,
// OpenCV's adaptive iteration count, a fixed-tree block sum, the finite-row test and register Gauss-Jordan.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"
#include "sampling.h"

// nothing here is fused: the numpy restatements (tools/geometry_ref.py, tools/essential_ref.py) evaluate the same expressions
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int MAX_TRY = 64;           // redraws of one sample index before the sample is given up
constexpr double PIVOT_EPS = 1e-6;      // |pivot| of the minimal solvers' elimination (normalised coordinates)

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

}  // namespace
}  // namespace roma
