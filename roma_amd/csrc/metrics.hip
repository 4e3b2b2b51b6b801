// Scoring tail of the pose and homography benchmarks: the reference's compute_pose_error and pose_auc (romatch/utils/utils.py), the
// accuracy / mAP lines of its MegaDepth and ScanNet pose benchmarks and the corner distance of its HPatches benchmark, so that a
// loop of estimate_pose / find_homography calls is scored without reading R, t, ok back.  The definition is stated in
// include/roma_hip.h and restated, operation by operation, in numpy float64 by tools/metrics_ref.py - the oracle of
// tests/test_gpu_metrics.py.
//
// Four kernels, each ONE workgroup (a pair is a few dozen float64 operations; a call is bounded by its launch):
//   1. pose_error_kernel        a pair per thread: (e_t, e_R, e_pose) in degrees, 90 for a pair without a pose;
//   2. corner_error_kernel      a pair per thread: the four corners through both homographies, mean distance over min(w2, h2) / 480;
//   3. error_log_append_kernel  B values already on the device into the log;
//   4. error_summary_kernel     per threshold: count, sum and maximum of the errors below it - per thread in ascending index, a
//                               shuffle tree over the wave, the waves in order (as dense_metrics_kernel) - then accuracy and the
//                               closed form of pose_auc.
// The error log is device memory, double rows[capacity] and long long state[2] = {count, dropped}.  Kernels 1 - 3 append to it in
// the launch that computes the rows: every thread reads count, row i goes to count + i where that is below capacity, and after a
// barrier thread 0 stores count + B and adds what did not fit to dropped.  One workgroup per launch, so there is no other reader
// or writer of the cursor inside a launch, and successive launches order themselves by the stream: no host value takes part, no
// atomic is used.  No float is added atomically, nothing is read back.
#include <math.h>
#include <stdint.h>

#include "../../include/roma_hip.h"
#include "common.h"

// nothing here is fused: tools/metrics_ref.py evaluates the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_MAX_B = 65535;
constexpr int MT_MAX_THRESHOLDS = 16;
constexpr long MT_MAX_ERRORS = 65536;
constexpr double MT_RAD2DEG = 180.0 / 3.14159265358979323846;  // numpy's rad2deg: x * (180.0 / pi)

struct Log {
  double* rows;
  long long capacity;
  long long* state;  // {count, dropped}
};

__device__ __forceinline__ long long log_count(const Log& g) { return g.rows ? g.state[0] : 0; }

__device__ __forceinline__ void log_put(const Log& g, long long count, int i, double v) {
  const long long at = count + i;
  if (at >= 0 && at < g.capacity) g.rows[at] = v;
}

// the whole workgroup, after its rows are written: thread 0 moves the cursor.  The barrier also keeps every thread's read of
// count ahead of this store.
__device__ __forceinline__ void log_advance(const Log& g, long long count, int B) {
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long end = count + B;
  const long long kept_to = count > g.capacity ? count : g.capacity;  // rows at or beyond capacity were not written
  g.state[0] = end;
  if (end > kept_to) g.state[1] = g.state[1] + (end - kept_to);
}

__device__ __forceinline__ double clip1(double c) { return c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c); }  // NaN stays, as in np.clip

struct PoseParams {
  const double* R;
  const double* t;
  const unsigned char* ok;
  const double* T;
  int t_rows, B;
  double* err;
  Log log;
};

__global__ __launch_bounds__(MT_THREADS) void pose_error_kernel(const PoseParams A) {
  const long long count = log_count(A.log);
  for (int b = threadIdx.x; b < A.B; b += MT_THREADS) {
    double e_t = 90.0, e_R = 90.0;
    if (!A.ok || A.ok[b]) {
      const double* r = A.R + (long)b * 9;
      const double* t = A.t + (long)b * 3;
      const double* g = A.T + (long)b * A.t_rows * 4;
      const double t0 = t[0], t1 = t[1], t2 = t[2];
      const double g0 = g[3], g1 = g[7], g2 = g[11];
      // angle_error_vec, then the ambiguity of the sign of t
      const double n = sqrt((t0 * t0 + t1 * t1) + t2 * t2) * sqrt((g0 * g0 + g1 * g1) + g2 * g2);
      const double ct = clip1(((t0 * g0 + t1 * g1) + t2 * g2) / n);
      const double a = acos(ct) * MT_RAD2DEG;
      const double f = 180.0 - a;
      e_t = f < a ? f : a;  // np.minimum: a NaN stays
      // angle_error_mat: trace(R^T R_gt) is the sum of the nine products, in row-major order
      double tr = r[0] * g[0];
      tr = tr + r[1] * g[1];
      tr = tr + r[2] * g[2];
      tr = tr + r[3] * g[4];
      tr = tr + r[4] * g[5];
      tr = tr + r[5] * g[6];
      tr = tr + r[6] * g[8];
      tr = tr + r[7] * g[9];
      tr = tr + r[8] * g[10];
      e_R = fabs(acos(clip1((tr - 1.0) / 2.0))) * MT_RAD2DEG;
    }
    const double e_pose = e_R > e_t ? e_R : e_t;  // Python's max(e_t, e_R): a NaN e_t stays
    double* o = A.err + (long)b * 3;
    o[0] = e_t, o[1] = e_R, o[2] = e_pose;
    if (A.log.rows) log_put(A.log, count, b, e_pose);
  }
  if (A.log.rows) log_advance(A.log, count, A.B);
}

struct Point {
  double x, y;
};

// row-vector corner (x, y, 1) times H^T, then the division by the third coordinate (inf / NaN of a zero one propagate)
__device__ __forceinline__ Point through(const double* h, double x, double y) {
  const double X = (h[0] * x + h[1] * y) + h[2];
  const double Y = (h[3] * x + h[4] * y) + h[5];
  const double Z = (h[6] * x + h[7] * y) + h[8];
  return {X / Z, Y / Z};
}

struct CornerParams {
  const double* Hp;
  const unsigned char* ok;
  const double* Hg;
  const double* sizes;
  int B;
  double* err;
  Log log;
};

__global__ __launch_bounds__(MT_THREADS) void corner_error_kernel(const CornerParams A) {
  const long long count = log_count(A.log);
  for (int b = threadIdx.x; b < A.B; b += MT_THREADS) {
    double hp[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};  // the reference's stand-in for a failed estimate
    if (!A.ok || A.ok[b]) {
#pragma unroll
      for (int q = 0; q < 9; ++q) hp[q] = A.Hp[(long)b * 9 + q];
    }
    double hg[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) hg[q] = A.Hg[(long)b * 9 + q];
    const double* sz = A.sizes + (long)b * 4;
    const double xe = sz[0] - 1.0, ye = sz[1] - 1.0;
    const double cx[4] = {0.0, 0.0, xe, xe}, cy[4] = {0.0, ye, 0.0, ye};
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const Point real = through(hg, cx[c], cy[c]), pred = through(hp, cx[c], cy[c]);
      const double dx = real.x - pred.x, dy = real.y - pred.y;
      const double d = sqrt(dx * dx + dy * dy);
      sum = sum + d;
    }
    const double side = sz[2] < sz[3] ? sz[2] : sz[3];
    const double e = (sum / 4.0) / (side / 480.0);
    A.err[b] = e;
    if (A.log.rows) log_put(A.log, count, b, e);
  }
  if (A.log.rows) log_advance(A.log, count, A.B);
}

__global__ __launch_bounds__(MT_THREADS) void error_log_append_kernel(const double* values, int B, const Log log) {
  const long long count = log_count(log);
  for (int b = threadIdx.x; b < B; b += MT_THREADS) log_put(log, count, b, values[b]);
  log_advance(log, count, B);
}

struct SummaryParams {
  const double* errors;
  long long n;
  const long long* state;  // non-null: n = min(state[0], capacity), read here
  long long capacity;
  int T;
  double thr[MT_MAX_THRESHOLDS];
  long long* out_n;
  long long* below;
  double* acc;
  double* auc;
};

__global__ __launch_bounds__(MT_THREADS) void error_summary_kernel(const SummaryParams A) {
  __shared__ double s_sum[MT_WAVES], s_max[MT_WAVES];
  __shared__ int s_cnt[MT_WAVES];
  long long n = A.n;
  if (A.state) {
    n = A.state[0];
    n = n < 0 ? 0 : (n > A.capacity ? A.capacity : n);
  }
  const int wave = threadIdx.x >> 6;
  for (int k = 0; k < A.T; ++k) {
    const double thr = A.thr[k];
    // the errors strictly below the threshold: how many, their sum, their maximum (0 when there is none); NaN and +inf are never below
    int L = 0;
    double S = 0.0, M = 0.0;
    for (long long i = threadIdx.x; i < n; i += MT_THREADS) {
      const double e = A.errors[i];
      if (e < thr) {
        L += 1;
        S = S + e;
        M = e > M ? e : M;
      }
    }
    // fixed tree over the wave, then the waves in order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      L += __shfl_down(L, off);
      S = S + __shfl_down(S, off);
      const double m = __shfl_down(M, off);
      M = m > M ? m : M;
    }
    if ((threadIdx.x & 63) == 0) s_cnt[wave] = L, s_sum[wave] = S, s_max[wave] = M;
    __syncthreads();
    if (threadIdx.x == 0) {
      int l = s_cnt[0];
      double s = s_sum[0], m = s_max[0];
      for (int v = 1; v < MT_WAVES; ++v) {
        l += s_cnt[v];
        s = s + s_sum[v];
        m = s_max[v] > m ? s_max[v] : m;
      }
      // the trapezoid under the recall curve from 0 to thr, telescoped; no error at all: 0 / 0 = NaN
      const double N = (double)n;
      A.below[k] = (long long)l;
      A.acc[k] = (double)l / N;
      A.auc[k] = ((((double)l * thr) - s) + m / 2.0) / (N * thr);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) A.out_n[0] = n;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// the checks the three appending entries share; log NULL: no log
const char* log_fault(const double* log, long capacity, const long long* state) {
  if (!log && !state) return nullptr;
  if (!log || !state) return "the error log needs both its rows and its state";
  if (capacity < 1) return "the capacity of the error log must be at least 1";
  if (!aligned8(log) || !aligned8(state)) return "the error log is not 8-byte aligned";
  return nullptr;
}

}  // namespace

extern "C" int roma_op_pose_error(const double* R, const double* t, const unsigned char* ok, const double* T_gt, int t_rows, int B,
                                  double* err, double* log, long capacity, long long* state, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(R && t && T_gt && err, "pose_error: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= MT_MAX_B, "pose_error: B must lie in [0, 65535]");
  ROMA_REQUIRE(t_rows == 3 || t_rows == 4, "pose_error: t_rows must be 3 ([B, 3, 4]) or 4 ([B, 4, 4])");
  ROMA_REQUIRE(aligned8(R) && aligned8(t) && aligned8(T_gt) && aligned8(err), "pose_error: a float64 array is not 8-byte aligned");
  if (const char* fault = log_fault(log, capacity, state)) ROMA_REQUIRE(false, std::string("pose_error: ") + fault);
  if (B == 0) return 0;
  PoseParams A = {R, t, ok, T_gt, t_rows, B, err, {log, capacity, state}};
  ProfScope ps("pose_error_kernel", (double)B * 200.0, "B", s);
  hipLaunchKernelGGL(pose_error_kernel, dim3(1), dim3(MT_THREADS), 0, s, A);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_corner_error(const double* H_pred, const unsigned char* ok, const double* H_gt, const double* sizes, int B,
                                    double* err, double* log, long capacity, long long* state, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(H_pred && H_gt && sizes && err, "corner_error: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= MT_MAX_B, "corner_error: B must lie in [0, 65535]");
  ROMA_REQUIRE(aligned8(H_pred) && aligned8(H_gt) && aligned8(sizes) && aligned8(err),
               "corner_error: a float64 array is not 8-byte aligned");
  if (const char* fault = log_fault(log, capacity, state)) ROMA_REQUIRE(false, std::string("corner_error: ") + fault);
  if (B == 0) return 0;
  CornerParams A = {H_pred, ok, H_gt, sizes, B, err, {log, capacity, state}};
  ProfScope ps("corner_error_kernel", (double)B * 184.0, "B", s);
  hipLaunchKernelGGL(corner_error_kernel, dim3(1), dim3(MT_THREADS), 0, s, A);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_error_log_append(const double* values, int B, double* log, long capacity, long long* state, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(values && log && state, "error_log_append: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= MT_MAX_B, "error_log_append: B must lie in [0, 65535]");
  ROMA_REQUIRE(aligned8(values), "error_log_append: values is not 8-byte aligned");
  if (const char* fault = log_fault(log, capacity, state)) ROMA_REQUIRE(false, std::string("error_log_append: ") + fault);
  if (B == 0) return 0;
  Log g = {log, capacity, state};
  ProfScope ps("error_log_append_kernel", (double)B * 16.0, "B", s);
  hipLaunchKernelGGL(error_log_append_kernel, dim3(1), dim3(MT_THREADS), 0, s, values, B, g);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_error_summary(const double* errors, long n, const long long* state, long capacity, const double* thresholds_host,
                                     int T, long long* out_n, long long* out_below, double* out_acc, double* out_auc, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(thresholds_host && out_n && out_below && out_acc && out_auc, "error_summary: null pointer");
  ROMA_REQUIRE(T >= 1 && T <= MT_MAX_THRESHOLDS, "error_summary: the number of thresholds must lie in [1, 16]");
  if (state) {
    ROMA_REQUIRE(capacity >= 1 && capacity <= MT_MAX_ERRORS, "error_summary: one summary takes at most 65536 errors (the log's capacity)");
    ROMA_REQUIRE(errors, "error_summary: null pointer");
    ROMA_REQUIRE(aligned8(state), "error_summary: state is not 8-byte aligned");
  } else {
    ROMA_REQUIRE(n >= 0 && n <= MT_MAX_ERRORS, "error_summary: one summary takes at most 65536 errors");
    ROMA_REQUIRE(errors || n == 0, "error_summary: null pointer");
  }
  ROMA_REQUIRE(aligned8(errors) && aligned8(out_n) && aligned8(out_below) && aligned8(out_acc) && aligned8(out_auc),
               "error_summary: an array is not 8-byte aligned");
  SummaryParams A = {};
  A.errors = errors, A.n = state ? 0 : n, A.state = state, A.capacity = state ? capacity : 0, A.T = T;
  for (int k = 0; k < T; ++k) {
    ROMA_REQUIRE(thresholds_host[k] > 0 && thresholds_host[k] <= 1.7976931348623157e308, "error_summary: a threshold is not positive and finite");
    A.thr[k] = thresholds_host[k];
  }
  A.out_n = out_n, A.below = out_below, A.acc = out_acc, A.auc = out_auc;
  ProfScope ps("error_summary_kernel", (double)(state ? capacity : n) * T * 8.0, "B", s);
  hipLaunchKernelGGL(error_summary_kernel, dim3(1), dim3(MT_THREADS), 0, s, A);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
