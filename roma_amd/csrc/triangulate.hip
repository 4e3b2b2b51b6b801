// Depth and 3-D points of matches under a known relative pose (roma_op_triangulate), and the mutual check of the two halves of a
// symmetric warp (roma_op_depth_consistency).  The definition is stated in include/roma_hip.h and restated, operation by
// operation, in numpy float64 by tools/triangulate_ref.py - the oracle of tests/test_gpu_triangulate.py.
//
// One-sided error model of a dense matcher: the pixel on the grid of the reference image is exact, the predicted coordinate in
// the other image carries the error.  The point lies on the reference pixel's ray, at the depth whose projection into the
// other image is closest to the prediction: the foot of the prediction on the ray's epipolar line.
//
// Both kernels stream: one 16-byte load per point (triangulate), plain vector stores, a grid-stride loop over a capped grid with
// the pair as the grid's y axis, so the pose and the cameras of a pair are wave-uniform loads.  No LDS, no workspace.  The only
// atomics are the integer counters of `stats`, whose totals do not depend on arrival order: every output is bit-identical from
// run to run and independent of B and of where the pair sits in the batch.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "common.h"
#include "triangulate.h"

// nothing here is fused: tools/triangulate_ref.py evaluates the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int TRI_THREADS = 256;
constexpr int TRI_MAX_BLOCKS = 2048;  // whole grid: 256 CUs x 8 workgroups; the rest is the grid-stride loop
constexpr double RAD_TO_DEG = 57.29577951308232;  // 180 / pi

struct Cam {
  double fx, fy, cx, cy;
};

struct Pose {  // maps reference-frame points to the other frame
  double r[9], t[3];
};

// what one half needs: its pose, the reference and the other camera, the epipole Bv = K_o t and both image sizes
struct View {
  Pose p;
  Cam ref, oth;
  double bv0, bv1;  // Bv2 = t2
  int w_ref, h_ref, w_oth, h_oth;
};

struct TriParams {
  const float* matches;
  const float* certainty;
  const int* counts;
  const unsigned char* valid;
  const double* R;
  const double* t;
  const double* K_a;
  const double* K_b;
  long n;
  int coords, sym_w;
  int W_a, H_a, W_b, H_b;
  double max_depth, max_reproj, min_parallax, min_certainty;
  float* points;
  float* depth_other;
  float* reproj;
  float* parallax;
  unsigned char* flags;
  int* stats;
};

__device__ __forceinline__ Cam load_cam(const double* K, int b) {
  Cam c = {1.0, 1.0, 0.0, 0.0};
  if (K) {
    const double* k = K + (long)b * 9;
    c.fx = k[0], c.fy = k[4], c.cx = k[2], c.cy = k[5];
  }
  return c;
}

__device__ __forceinline__ bool finite_cam(const Cam& c) { return isfinite(c.fx) && isfinite(c.fy) && isfinite(c.cx) && isfinite(c.cy); }

__device__ __forceinline__ Pose load_pose(const double* R, const double* t, int b) {
  Pose p;
#pragma unroll
  for (int i = 0; i < 9; ++i) p.r[i] = R[(long)b * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) p.t[i] = t[(long)b * 3 + i];
  return p;
}

// (R^T, -R^T t)
__device__ __forceinline__ Pose inverse_pose(const Pose& p) {
  Pose q;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) q.r[i * 3 + k] = p.r[k * 3 + i];
    q.t[i] = -((p.r[0 * 3 + i] * p.t[0] + p.r[1 * 3 + i] * p.t[1]) + p.r[2 * 3 + i] * p.t[2]);
  }
  return q;
}

__device__ __forceinline__ bool finite_pose(const Pose& p) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && isfinite(p.r[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) ok = ok && isfinite(p.t[i]);
  return ok;
}

// The float64 chain (atan2's polynomial above all) keeps more wave-uniform values live than a wave has scalar registers.  The
// ones below are parked in vector registers, which the kernel has to spare, so that no scalar register is spilled.
__device__ __forceinline__ void park(double* x) { asm volatile("" : "+v"(*x)); }

__device__ __forceinline__ void set_epipole(View* v) {
  v->bv0 = v->oth.fx * v->p.t[0] + v->oth.cx * v->p.t[2];
  v->bv1 = v->oth.fy * v->p.t[1] + v->oth.cy * v->p.t[2];
}

struct TriOut {
  float x, y, z, z_other, reproj, parallax;
  unsigned flag;
};

// one point: (u, v) the reference pixel or normalised coordinate, (uo, vo) the observation in the other image.  count[7]:
// {considered, valid, degenerate, cheirality, reproj, parallax, certainty} of this thread and half.
__device__ __forceinline__ TriOut tri_point(const View& V, const TriParams& P, bool pose_ok, double u, double v, double uo, double vo,
                                            bool has_cert, double cert, int (&count)[7]) {
  const float nanf_ = __int_as_float(0x7fc00000);
  TriOut o = {nanf_, nanf_, nanf_, nanf_, nanf_, nanf_, TRI_DEGENERATE};
  count[0] += 1;
  const bool finite_in = isfinite(u) && isfinite(v) && isfinite(uo) && isfinite(vo);
  if (P.coords) {
    u = (u + 1.0) * (double)V.w_ref / 2.0, v = (v + 1.0) * (double)V.h_ref / 2.0;
    uo = (uo + 1.0) * (double)V.w_oth / 2.0, vo = (vo + 1.0) * (double)V.h_oth / 2.0;
  }
  // ray images
  const double x0 = (u - V.ref.cx) / V.ref.fx, x1 = (v - V.ref.cy) / V.ref.fy;
  const double r0 = (V.p.r[0] * x0 + V.p.r[1] * x1) + V.p.r[2];
  const double r1 = (V.p.r[3] * x0 + V.p.r[4] * x1) + V.p.r[5];
  const double r2 = (V.p.r[6] * x0 + V.p.r[7] * x1) + V.p.r[8];
  const double A0 = V.oth.fx * r0 + V.oth.cx * r2, A1 = V.oth.fy * r1 + V.oth.cy * r2, A2 = r2;
  // epipolar line of the reference pixel, signed residual and foot point of the observation
  const double bv2 = V.p.t[2];
  const double l0 = A1 * bv2 - A2 * V.bv1, l1 = A2 * V.bv0 - A0 * bv2, l2 = A0 * V.bv1 - A1 * V.bv0;
  const double n2 = l0 * l0 + l1 * l1;
  if (!(pose_ok && finite_in && n2 > 0.0)) {
    count[2] += 1;
    return o;
  }
  const double s = (l0 * uo + l1 * vo) + l2;
  const double d = s / sqrt(n2);
  const double px = uo - (s * l0) / n2, py = vo - (s * l1) / n2;
  // depth along the ray
  const double a0 = px * A2 - A0, a1 = py * A2 - A1;
  const double b0 = V.bv0 - px * bv2, b1 = V.bv1 - py * bv2;
  const double lam = a0 * b0 + a1 * b1, w = a0 * a0 + a1 * a1;
  const double z = lam / w;
  const double zo = z * r2 + V.p.t[2];
  // parallax
  const double h0 = (px - V.oth.cx) / V.oth.fx, h1 = (py - V.oth.cy) / V.oth.fy;
  const double c0 = r1 - r2 * h1, c1 = r2 * h0 - r0, c2 = r0 * h1 - r1 * h0;
  const double cn = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  const double dot = (r0 * h0 + r1 * h1) + r2;
  const double par = atan2(cn, dot) * RAD_TO_DEG;

  unsigned f = 0;
  if (!(z > 0.0 && z < P.max_depth) || !(zo > 0.0 && zo < P.max_depth)) f |= TRI_CHEIRALITY, count[3] += 1;
  if (!(fabs(d) <= P.max_reproj)) f |= TRI_REPROJ, count[4] += 1;
  if (!(par >= P.min_parallax)) f |= TRI_PARALLAX, count[5] += 1;
  if (has_cert && !(cert >= P.min_certainty)) f |= TRI_CERTAINTY, count[6] += 1;
  if (f == 0) count[1] += 1;
  o.x = (float)(z * x0), o.y = (float)(z * x1), o.z = (float)z;
  o.z_other = (float)zo, o.reproj = (float)d, o.parallax = (float)par;
  o.flag = f;
  return o;
}

// grid (blocks, B, halves): a workgroup serves one pair and one half of the grid (halves = 2 for a symmetric warp, whose row of 2W
// points holds W A-reference and W B-reference points), so its pose, cameras and epipole are wave-uniform
__global__ __launch_bounds__(TRI_THREADS) void triangulate_kernel(const TriParams P) {
  const int b = blockIdx.y, half = blockIdx.z;
  const long n = P.n, base = (long)b * n;
  const bool pair_on = !P.valid || P.valid[b] != 0;
  long rows = 0;
  View V = {};
  bool pose_ok = false;
  if (pair_on) {
    rows = n;
    if (P.counts) rows = std::min<long>(std::max<long>((long)P.counts[b], 0), n);
    const Pose p = load_pose(P.R, P.t, b);
    const Cam ka = load_cam(P.K_a, b), kb = load_cam(P.K_b, b);
    pose_ok = finite_pose(p) && finite_cam(ka) && finite_cam(kb);
    if (!half) {
      V.p = p, V.ref = ka, V.oth = kb;
      V.w_ref = P.W_a, V.h_ref = P.H_a, V.w_oth = P.W_b, V.h_oth = P.H_b;
    } else {
      V.p = inverse_pose(p), V.ref = kb, V.oth = ka;
      V.w_ref = P.W_b, V.h_ref = P.H_b, V.w_oth = P.W_a, V.h_oth = P.H_a;
    }
    set_epipole(&V);
  }
  TriParams Q = P;  // thresholds
  park(&Q.max_depth), park(&Q.max_reproj), park(&Q.min_parallax), park(&Q.min_certainty);
  park(&V.bv0), park(&V.bv1), park(&V.p.t[2]);
  park(&V.oth.fx), park(&V.oth.fy), park(&V.oth.cx), park(&V.oth.cy);
  const unsigned W = (unsigned)P.sym_w;
  const long mine = W ? n / 2 : n;  // points of this half
  const bool has_cert = P.certainty != nullptr;
  const float nanf_ = __int_as_float(0x7fc00000);
  int count[7] = {0, 0, 0, 0, 0, 0, 0};
  const long stride = (long)gridDim.x * TRI_THREADS;
  for (long k = (long)blockIdx.x * TRI_THREADS + threadIdx.x; k < mine; k += stride) {
    // k-th point of this half -> row j of the pair: k < 2^30 where the grid has halves
    const long j = W ? (long)((unsigned)k / W) * (2 * W) + (half ? W : 0u) + (unsigned)k % W : k;
    TriOut o = {nanf_, nanf_, nanf_, nanf_, nanf_, nanf_, TRI_SKIPPED};
    if (j < rows) {
      const f32x4 m = *reinterpret_cast<const f32x4*>(P.matches + (base + j) * 4);
      const double cert = has_cert ? (double)P.certainty[base + j] : 0.0;
      if (!half) o = tri_point(V, Q, pose_ok, (double)m[0], (double)m[1], (double)m[2], (double)m[3], has_cert, cert, count);
      else o = tri_point(V, Q, pose_ok, (double)m[2], (double)m[3], (double)m[0], (double)m[1], has_cert, cert, count);
    }
    float* xyz = P.points + (base + j) * 3;
    xyz[0] = o.x, xyz[1] = o.y, xyz[2] = o.z;
    if (P.depth_other) P.depth_other[base + j] = o.z_other;
    if (P.reproj) P.reproj[base + j] = o.reproj;
    if (P.parallax) P.parallax[base + j] = o.parallax;
    P.flags[base + j] = (unsigned char)o.flag;
  }
  if (!P.stats) return;
  // one integer atomic per wave and counter
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    int v = count[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&P.stats[((long)b * 2 + half) * 8 + c], v);
  }
}

struct ConsParams {
  const float* points;
  const unsigned char* flags;
  const double* R;
  const double* t;
  const double* K_a;
  const double* K_b;
  int W_a, H_a, W_b, H_b, H, W;
  double rel_thresh;
  unsigned char* consistent;
  float* err;
};

// grid (blocks, B) over the [H, 2W] points of a pair
__global__ __launch_bounds__(TRI_THREADS) void depth_consistency_kernel(const ConsParams P) {
  const int b = blockIdx.y;
  const unsigned W = (unsigned)P.W, W2 = 2u * W;
  const long n = (long)P.H * W2, base = (long)b * n;
  const Pose p = load_pose(P.R, P.t, b);
  const Cam ka = load_cam(P.K_a, b), kb = load_cam(P.K_b, b);
  const double gw = (double)P.W, gh = (double)P.H;
  const float nanf_ = __int_as_float(0x7fc00000);
  const long stride = (long)gridDim.x * TRI_THREADS;
  for (long j = (long)blockIdx.x * TRI_THREADS + threadIdx.x; j < n; j += stride) {
    unsigned char out = 2;
    float e_out = nanf_;
    if (P.flags[base + j] == 0) {
      const bool is_b = (unsigned)j % W2 >= W;  // j < 2^31
      const float* xyz = P.points + (base + j) * 3;
      const double X0 = (double)xyz[0], X1 = (double)xyz[1], X2 = (double)xyz[2];
      double y0, y1, y2;
      if (!is_b) {
        y0 = ((p.r[0] * X0 + p.r[1] * X1) + p.r[2] * X2) + p.t[0];
        y1 = ((p.r[3] * X0 + p.r[4] * X1) + p.r[5] * X2) + p.t[1];
        y2 = ((p.r[6] * X0 + p.r[7] * X1) + p.r[8] * X2) + p.t[2];
      } else {
        const double d0 = X0 - p.t[0], d1 = X1 - p.t[1], d2 = X2 - p.t[2];
        y0 = (p.r[0] * d0 + p.r[3] * d1) + p.r[6] * d2;
        y1 = (p.r[1] * d0 + p.r[4] * d1) + p.r[7] * d2;
        y2 = (p.r[2] * d0 + p.r[5] * d1) + p.r[8] * d2;
      }
      const Cam k = is_b ? ka : kb;
      const double wo = is_b ? (double)P.W_a : (double)P.W_b, ho = is_b ? (double)P.H_a : (double)P.H_b;
      const double px = k.fx * (y0 / y2) + k.cx, py = k.fy * (y1 / y2) + k.cy;
      const double gx = px / wo * gw - 0.5, gy = py / ho * gh - 0.5;
      const double fx0 = floor(gx), fy0 = floor(gy);
      // the four neighbours lie inside the other half (NaN fails every comparison)
      if (fx0 >= 0.0 && fx0 + 1.0 <= gw - 1.0 && fy0 >= 0.0 && fy0 + 1.0 <= gh - 1.0) {
        const long i00 = base + (long)fy0 * W2 + (is_b ? 0 : W) + (long)fx0, i10 = i00 + W2;
        if ((P.flags[i00] | P.flags[i00 + 1] | P.flags[i10] | P.flags[i10 + 1]) == 0) {
          const double d00 = (double)P.points[i00 * 3 + 2], d01 = (double)P.points[(i00 + 1) * 3 + 2];
          const double d10 = (double)P.points[i10 * 3 + 2], d11 = (double)P.points[(i10 + 1) * 3 + 2];
          const double ax = gx - fx0, ay = gy - fy0;
          const double v = (d00 * (1.0 - ax) + d01 * ax) * (1.0 - ay) + (d10 * (1.0 - ax) + d11 * ax) * ay;
          const double e = fabs(v - y2) / v;
          out = e < P.rel_thresh ? 1 : 0;
          e_out = (float)e;
        }
      }
    }
    P.consistent[base + j] = out;
    if (P.err) P.err[base + j] = e_out;
  }
}

unsigned grid_x(long n, int B) {
  const long want = (n + TRI_THREADS - 1) / TRI_THREADS;
  return (unsigned)std::max<long>(1, std::min<long>(want, std::max(1, TRI_MAX_BLOCKS / B)));
}

}  // namespace

extern "C" int roma_op_triangulate(const float* matches, const float* certainty, const int* counts, const unsigned char* valid,
                                   const double* R, const double* t, const double* K_a, const double* K_b, int B, long n, int coords,
                                   int W_a, int H_a, int W_b, int H_b, int sym_w, double max_depth, double max_reproj, double min_parallax,
                                   double min_certainty, float* points, float* depth_other, float* reproj, float* parallax,
                                   unsigned char* flags, int* stats, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(matches && R && t && points && flags, "triangulate: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "triangulate: B must lie in [0, 65535]");
  ROMA_REQUIRE(n >= 0, "triangulate: n must not be negative");
  ROMA_REQUIRE(B == 0 || n < (1l << 31) / B + ((1l << 31) % B != 0), "triangulate: B * n must be below 2^31");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(matches) & 15) == 0, "triangulate: matches must be 16-byte aligned");
  ROMA_REQUIRE(coords == 0 || coords == 1, "triangulate: coords must be 0 (pixels) or 1 (normalised)");
  ROMA_REQUIRE(sym_w >= 0 && (sym_w == 0 || (sym_w <= (1 << 30) && n % (2l * sym_w) == 0)),
               "triangulate: sym_w must be 0 or W with n a multiple of 2 W");
  ROMA_REQUIRE(coords == 0 || (W_a > 0 && H_a > 0 && W_b > 0 && H_b > 0), "triangulate: coords = 1 needs positive image sizes");
  ROMA_REQUIRE(max_depth >= 0 && max_reproj >= 0 && min_parallax >= 0 && min_certainty >= 0,
               "triangulate: a threshold is negative (or NaN)");
  if (B == 0 || n == 0) return 0;
  if (stats) ROMA_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)B * 16 * sizeof(int), s));
  TriParams P = {matches, certainty, counts, valid, R, t, K_a, K_b, n, coords, sym_w, W_a, H_a, W_b, H_b, max_depth, max_reproj,
                 min_parallax, min_certainty, points, depth_other, reproj, parallax, flags, stats};
  ProfScope ps("triangulate_kernel", (double)B * (double)n * 45.0, "B", s);
  const int halves = sym_w ? 2 : 1;
  hipLaunchKernelGGL(triangulate_kernel, dim3(grid_x(n / halves, B * halves), B, halves), dim3(TRI_THREADS), 0, s, P);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int roma_op_depth_consistency(const float* points, const unsigned char* flags, const double* R, const double* t,
                                         const double* K_a, const double* K_b, int W_a, int H_a, int W_b, int H_b, int B, int H, int W,
                                         double rel_thresh, unsigned char* consistent, float* err, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(points && flags && R && t && consistent, "depth_consistency: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "depth_consistency: B must lie in [0, 65535]");
  ROMA_REQUIRE(H >= 0 && W >= 0, "depth_consistency: H and W must not be negative");
  ROMA_REQUIRE(W_a > 0 && H_a > 0 && W_b > 0 && H_b > 0, "depth_consistency: image sizes must be positive");
  ROMA_REQUIRE(rel_thresh >= 0, "depth_consistency: rel_thresh is negative (or NaN)");
  if (B == 0 || H == 0 || W == 0) return 0;
  ROMA_REQUIRE(W <= (1 << 30) && (long)H * (2l * W) < (1l << 31) / B + ((1l << 31) % B != 0),
               "depth_consistency: B * H * 2 W must be below 2^31");
  const long n = (long)H * 2 * W;
  ConsParams P = {points, flags, R, t, K_a, K_b, W_a, H_a, W_b, H_b, H, W, rel_thresh, consistent, err};
  ProfScope ps("depth_consistency_kernel", (double)B * (double)n * 18.0, "B", s);
  hipLaunchKernelGGL(depth_consistency_kernel, dim3(grid_x(n, B), B), dim3(TRI_THREADS), 0, s, P);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
