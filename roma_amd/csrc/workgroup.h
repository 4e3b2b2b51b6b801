// Integer count, sum, scan and rank over the threads of a one-dimensional workgroup: what the geometry operators' count -> scan ->
// rank compaction is made of.  Device-only.  WAVES is the workgroup's number of waves, a template argument so that the loops over
// the wave totals unroll; the LDS scratch is the caller's, WAVES elements.  Every thread of the workgroup calls a wg_ function (they
// hold barriers), every thread of the wave a wave_ function.  All of it is integer arithmetic: the results do not depend on the
// schedule.
#pragma once
#include <hip/hip_runtime.h>

namespace roma {

constexpr int WAVE = 64;  // lanes of a wave on gfx950

// the number of set bits of a wave's ballot below the calling lane
__device__ __forceinline__ int wave_rank(unsigned long long ballot) {
  return __popcll(ballot & ((1ull << (threadIdx.x & (WAVE - 1))) - 1ull));
}

// *dst += the wave's number of pred: one atomic per wave that has something to count
__device__ __forceinline__ void wave_count_add(int* dst, bool pred) {
  const int n = __popcll(__ballot(pred));
  if (n && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(dst, n);
}

// The workgroup's number of pred, in thread 0 only (the other threads get 0).  Two barriers: the second frees wc for the next call.
template <int WAVES>
__device__ __forceinline__ int wg_count(bool pred, int* wc) {
  const int n = __popcll(__ballot(pred));
  if ((threadIdx.x & (WAVE - 1)) == 0) wc[threadIdx.x / WAVE] = n;
  __syncthreads();
  int s = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += wc[w];
  }
  __syncthreads();
  return s;
}

// *dst += the workgroup's number of pred: one atomic per workgroup that has something to count, the waves' ballots meet in LDS
// first.  (One per wave was measured in depth fusion: 93 000 waves adding to the two counters of one problem took 2 ms a kernel,
// forty times the rest of its work.)
template <int WAVES>
__device__ __forceinline__ void wg_count_add(int* dst, bool pred, int* wc) {
  const int n = __popcll(__ballot(pred));
  if ((threadIdx.x & (WAVE - 1)) == 0) wc[threadIdx.x / WAVE] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += wc[w];
    if (s) atomicAdd(dst, s);
  }
  __syncthreads();  // frees wc for the next call
}

// the sum of v over the workgroup, the same in every thread; may be called again on the same sh
template <int WAVES>
__device__ __forceinline__ int wg_sum(int v, int* sh) {
#pragma unroll
  for (int off = WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();  // the previous call's readers are done with sh
  if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x / WAVE] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += sh[w];
  return s;
}

// The exclusive prefix of v in thread order, and the workgroup's total in every thread; the inclusive prefix is the result + v.
// T is int, unsigned or long long.  A shuffle scan per wave, the wave totals through LDS: two barriers, the first in front of the
// LDS write, so that it may be called again on the same wt (a chunked walk with a carry does).
template <int WAVES, typename T>
__device__ __forceinline__ T wg_scan_exclusive(T v, T* wt, T& total) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  T inc = v;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const T up = __shfl_up(inc, off);
    inc += lane >= off ? up : 0;
  }
  __syncthreads();  // the previous call's readers are done with wt
  if (lane == WAVE - 1) wt[wave] = inc;
  __syncthreads();
  T before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const T t = wt[w];
    before += w < wave ? t : 0;
    total += t;
  }
  return before + inc - v;
}

// The rank of a thread with pred among the threads with pred, in thread order (0 in a thread without), and their number in every
// thread: the ballot, the wave totals through LDS, the sum of the earlier waves.  Only the threads with pred walk the earlier
// waves: where few cells of a grid hold anything, most waves have nothing to do after the barrier (measured in set keypoints:
// without the guard skp_number took 80 us instead of 77.5).  One barrier: wc must not be in use when the workgroup arrives.
template <int WAVES>
__device__ __forceinline__ int wg_rank(bool pred, int* wc, int& total) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const unsigned long long bal = __ballot(pred);
  if (lane == 0) wc[wave] = __popcll(bal);
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) total += wc[w];
  int rank = 0;
  if (pred) {
    rank = wave_rank(bal);
#pragma unroll
    for (int w = 0; w < WAVES; ++w) rank += w < wave ? wc[w] : 0;
  }
  return rank;
}

}  // namespace roma
