// Dense multi-view depth fusion (roma_op_fuse_depth_maps): the P pairs of V <= 8 views give every view up to 14 depth
// hypotheses per pixel (the halves of roma_op_triangulate's output that lie on its grid); a vote selects among them, the fused
// maps check one another across views, duplicates of a surface point seen from several views are dropped and what stays is
// numbered into one point cloud.  The definition is in include/roma_hip.h; tools/depth_fusion_ref.py restates it in numpy
// float64, operation by operation, and is the oracle of tests/test_gpu_depth_fusion.py.  Also roma_op_relative_poses, the pose of
// every pair from the poses of the views.
//
// One thread per pixel throughout, grid (blocks of 256 pixels, view, problem): a workgroup never straddles two views, so the
// slot list of its view is wave-uniform and the cameras and poses are staged once per workgroup in LDS.  Five kernels on the
// stream, every phase closed by a kernel boundary - what one kernel decides is read only by the next:
//   select   the vote over the slots of a pixel: depth, weight, support
//   check    every fused pixel is moved into the other views and compared with their fused depth: seen, violated, keep
//   dedupe   a kept pixel is a duplicate when a lower view that sees it keeps the pixel nearest its projection - decided from
//            check's keep alone; state is written and every block counts what it emits
//   scan     one workgroup per problem: the exclusive prefix of the block counts in block order, counts and total
//   emit     the index of an emitted pixel is its block's prefix plus its rank inside the block (ballots, wave order): (view,
//            row-major pixel) order whatever the schedule; the cloud and its padding are written
// The only atomics are the integer counters of `stats`, one per workgroup that has something to count.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "pair_views.h"
#include "workgroup.h"
#include "workspace.h"

// nothing here is fused: tools/depth_fusion_ref.py evaluates the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int FUSE_MAX_VIEWS = 8, FUSE_MAX_PAIRS = 64;
constexpr int FUSE_MAX_SLOTS = 2 * (FUSE_MAX_VIEWS - 1);  // hypotheses of one view: (i, j) and (j, i) may both occur
constexpr int FUSE_STATS = 8;                              // ints per problem in roma_op_fuse_depth_maps' out_stats
constexpr int FUSE_MAX_COLOR_VIEWS = 128;                  // B * V with a colour source: offsets and sizes travel in the kernel's arguments
constexpr int FUSE_BLOCK = 256, FUSE_WAVES = FUSE_BLOCK / WAVE;
constexpr int FUSE_SCAN = 1024, FUSE_SCAN_WAVES = FUSE_SCAN / WAVE;

struct FuseParams {
  const float* points;
  const unsigned char* flags;
  const float* cert;
  const double* cam;
  const double* R;
  const double* t;
  const unsigned char* view_valid;
  const unsigned char* valid;
  int B, V, P, H, W, Wd;
  double rel;
  int min_support, min_consistent, max_violations, dedupe, max_points;
  float* depth;
  float* weight;
  unsigned char* support;
  unsigned char* seen;
  unsigned char* violated;
  unsigned char* state;
  float* out_points;
  unsigned char* out_colors;
  float* out_weight;
  int* out_source;
  int* counts;
  int* total;
  int* stats;
  unsigned char* keep;  // [B, V, H, W] workspace: check's decision
  int* bsum;            // [B, V nb] workspace: pixels a block emits, then their exclusive prefix
  int nb;               // blocks per view
  unsigned char nslots[FUSE_MAX_VIEWS];
  unsigned char slot[FUSE_MAX_VIEWS][FUSE_MAX_SLOTS];  // pair * 2 + half, ascending pair
  unsigned char pv[FUSE_MAX_PAIRS][2];
};

struct FuseColors {  // the colour source: host data, in the emit kernel's arguments
  const unsigned char* images;
  long long offset[FUSE_MAX_COLOR_VIEWS];
  int h[FUSE_MAX_COLOR_VIEWS], w[FUSE_MAX_COLOR_VIEWS];
};

struct FView {
  double fx, fy, cx, cy, r[9], t[3];
  int on;
};

__device__ __forceinline__ bool fuse_problem_on(const FuseParams& F, int b) { return !F.valid || F.valid[b] != 0; }
__device__ __forceinline__ bool fuse_view_on(const FuseParams& F, int b, int v) {
  return !F.view_valid || F.view_valid[(long)b * F.V + v] != 0;
}

// the views of problem b, once per workgroup
__device__ __forceinline__ void fuse_stage_views(const FuseParams& F, int b, FView* sv) {
  const int u = threadIdx.x;
  if (u < F.V) {
    const long at = (long)b * F.V + u;
    const double* k = F.cam + at * 9;
    FView w;
    w.fx = k[0], w.fy = k[4], w.cx = k[2], w.cy = k[5];
#pragma unroll
    for (int i = 0; i < 9; ++i) w.r[i] = F.R[at * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) w.t[i] = F.t[at * 3 + i];
    w.on = fuse_problem_on(F, b) && fuse_view_on(F, b, u) ? 1 : 0;
    sv[u] = w;
  }
  __syncthreads();
}

// X_w = R^T (z ((u - cx) / fx, (v - cy) / fy, 1) - t) of the centre of grid cell (r, c)
__device__ __forceinline__ void fuse_world(const FView& a, int r, int c, double z, double (&X)[3]) {
  const double x0 = (((double)c + 0.5) - a.cx) / a.fx, x1 = (((double)r + 0.5) - a.cy) / a.fy;
  const double d0 = z * x0 - a.t[0], d1 = z * x1 - a.t[1], d2 = z - a.t[2];
  X[0] = (a.r[0] * d0 + a.r[3] * d1) + a.r[6] * d2;
  X[1] = (a.r[1] * d0 + a.r[4] * d1) + a.r[7] * d2;
  X[2] = (a.r[2] * d0 + a.r[5] * d1) + a.r[8] * d2;
}

struct FProj {
  double z, gx, gy;  // depth in the view, position on its grid (align_corners = False: the centre of cell 0 is at 0)
};

__device__ __forceinline__ FProj fuse_project(const FView& u, const double (&X)[3]) {
  const double y0 = ((u.r[0] * X[0] + u.r[1] * X[1]) + u.r[2] * X[2]) + u.t[0];
  const double y1 = ((u.r[3] * X[0] + u.r[4] * X[1]) + u.r[5] * X[2]) + u.t[1];
  const double y2 = ((u.r[6] * X[0] + u.r[7] * X[1]) + u.r[8] * X[2]) + u.t[2];
  FProj p;
  p.z = y2;
  p.gx = (u.fx * (y0 / y2) + u.cx) - 0.5;
  p.gy = (u.fy * (y1 / y2) + u.cy) - 0.5;
  return p;
}

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_select_kernel(const FuseParams F) {
  __shared__ int wc[FUSE_WAVES];
  const int v = blockIdx.y, b = blockIdx.z;
  const int n = F.H * F.W, q = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  const bool in = q < n;
  const bool on = fuse_problem_on(F, b) && fuse_view_on(F, b, v);
  const int ns = on ? (int)F.nslots[v] : 0;  // the same in every thread of the workgroup
  const int r = in ? q / F.W : 0, c = in ? q - r * F.W : 0;
  double z[FUSE_MAX_SLOTS], w[FUSE_MAX_SLOTS], wz[FUSE_MAX_SLOTS];
  unsigned usable = 0;
#pragma unroll
  for (int s = 0; s < FUSE_MAX_SLOTS; ++s) {
    z[s] = 0.0, w[s] = 0.0, wz[s] = 0.0;
    if (s < ns) {
      const int code = F.slot[v][s], p = code >> 1, half = code & 1;
      const bool other_on = fuse_view_on(F, b, F.pv[p][1 - half]);
      if (in && other_on) {
        const long at = (((long)b * F.P + p) * F.H + r) * F.Wd + (half ? F.W : 0) + c;
        const unsigned char f = F.flags[at];
        const float zf = F.points[at * 3 + 2];
        const float wf = F.cert ? F.cert[at] : 1.0f;
        if (f == 0 && isfinite(zf) && zf > 0.0f && isfinite(wf) && wf > 0.0f) {
          usable |= 1u << s;
          z[s] = (double)zf, w[s] = (double)wf;
          wz[s] = w[s] * z[s];
        }
      }
    }
  }
  // the vote: the most supporters, then the largest weight, then the lowest slot
  int best_n = 0;
  double best_s = 0.0, best_num = 0.0;
#pragma unroll
  for (int k = 0; k < FUSE_MAX_SLOTS; ++k) {
    if (k < ns) {
      int nk = 0;
      double sk = 0.0, numk = 0.0;
#pragma unroll
      for (int l = 0; l < FUSE_MAX_SLOTS; ++l) {
        if (l < ns) {
          const bool sup = ((usable >> l) & 1u) && fabs(z[l] - z[k]) <= F.rel * fmin(z[l], z[k]);
          nk += sup ? 1 : 0;
          sk += sup ? w[l] : 0.0;
          numk += sup ? wz[l] : 0.0;
        }
      }
      if (((usable >> k) & 1u) && (nk > best_n || (nk == best_n && sk > best_s))) best_n = nk, best_s = sk, best_num = numk;
    }
  }
  const bool fused = best_n >= F.min_support;
  int* stats = F.stats + (long)b * FUSE_STATS;
  wg_count_add<FUSE_WAVES>(stats + 0, usable != 0, wc);
  wg_count_add<FUSE_WAVES>(stats + 1, in && fused, wc);
  if (!in) return;
  const long at = ((long)b * F.V + v) * n + q;
  F.depth[at] = fused ? (float)(best_num / best_s) : __int_as_float(0x7fc00000);
  F.weight[at] = fused ? (float)best_s : 0.0f;
  F.support[at] = (unsigned char)best_n;
}

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_check_kernel(const FuseParams F) {
  __shared__ FView sv[FUSE_MAX_VIEWS];
  __shared__ int wc[FUSE_WAVES];
  const int v = blockIdx.y, b = blockIdx.z;
  fuse_stage_views(F, b, sv);
  const int n = F.H * F.W, q = blockIdx.x * FUSE_BLOCK + threadIdx.x;
  const bool in = q < n;
  const long map0 = (long)b * F.V * n;
  const float zf = in ? F.depth[map0 + (long)v * n + q] : __int_as_float(0x7fc00000);
  const bool fused = !isnan(zf);
  unsigned seen = 0, violated = 0;
  if (fused) {
    const int r = q / F.W, c = q - r * F.W;
    const double gw = (double)F.W, gh = (double)F.H;
    double X[3];
    fuse_world(sv[v], r, c, (double)zf, X);
#pragma unroll 1
    for (int u = 0; u < F.V; ++u) {
      if (u == v || !sv[u].on) continue;
      const FProj p = fuse_project(sv[u], X);
      if (!(p.z > 0.0)) continue;
      const double fx0 = floor(p.gx), fy0 = floor(p.gy);
      // the four neighbours lie inside the grid (NaN fails every comparison)
      if (!(fx0 >= 0.0 && fx0 + 1.0 <= gw - 1.0 && fy0 >= 0.0 && fy0 + 1.0 <= gh - 1.0)) continue;
      const float* D = F.depth + map0 + (long)u * n + ((long)fy0 * F.W + (long)fx0);
      const float f00 = D[0], f01 = D[1], f10 = D[F.W], f11 = D[F.W + 1];
      if (isnan(f00) || isnan(f01) || isnan(f10) || isnan(f11)) continue;
      const double d00 = (double)f00, d01 = (double)f01, d10 = (double)f10, d11 = (double)f11;
      const double ax = p.gx - fx0, ay = p.gy - fy0;
      const double d = (d00 * (1.0 - ax) + d01 * ax) * (1.0 - ay) + (d10 * (1.0 - ax) + d11 * ax) * ay;
      const double e = (p.z - d) / d;
      if (fabs(e) <= F.rel) seen |= 1u << u;
      if (e < -F.rel) violated |= 1u << u;
    }
  }
  const bool keep = fused && __popc(seen) >= F.min_consistent && __popc(violated) <= F.max_violations;
  int* stats = F.stats + (long)b * FUSE_STATS;
  wg_count_add<FUSE_WAVES>(stats + 2, keep, wc);
  wg_count_add<FUSE_WAVES>(stats + 5, violated != 0, wc);
  if (!in) return;
  const long at = map0 + (long)v * n + q;
  F.seen[at] = (unsigned char)seen;
  F.violated[at] = (unsigned char)violated;
  F.keep[at] = keep ? 1 : 0;
}

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_dedupe_kernel(const FuseParams F) {
  __shared__ FView sv[FUSE_MAX_VIEWS];
  __shared__ int wcnt[FUSE_WAVES];
  const int v = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  fuse_stage_views(F, b, sv);
  const int n = F.H * F.W, q = blockIdx.x * FUSE_BLOCK + t;
  const bool in = q < n;
  const long map0 = (long)b * F.V * n, at = map0 + (long)v * n + q;
  const bool keep = in && F.keep[at] != 0;
  bool dup = false;
  if (keep && F.dedupe) {
    const unsigned seen = F.seen[at];
    const int r = q / F.W, c = q - r * F.W;
    const double gw = (double)F.W, gh = (double)F.H;
    double X[3];
    fuse_world(sv[v], r, c, (double)F.depth[at], X);
#pragma unroll 1
    for (int u = 0; u < v; ++u) {
      if (!((seen >> u) & 1u)) continue;
      const FProj p = fuse_project(sv[u], X);
      const double nx = floor(p.gx + 0.5), ny = floor(p.gy + 0.5);
      if (!(nx >= 0.0 && nx <= gw - 1.0 && ny >= 0.0 && ny <= gh - 1.0)) continue;
      if (F.keep[map0 + (long)u * n + ((long)ny * F.W + (long)nx)] != 0) dup = true;
    }
  }
  wg_count_add<FUSE_WAVES>(F.stats + (long)b * FUSE_STATS + 3, dup, wcnt);
  if (in) F.state[at] = (unsigned char)((keep ? 1 : 0) | (dup ? 2 : 0));
  const int cnt = wg_count<FUSE_WAVES>(keep && !dup, wcnt);
  if (t == 0) F.bsum[((long)b * F.V + v) * F.nb + blockIdx.x] = cnt;
}

// one workgroup per problem: bsum becomes its own exclusive prefix in block order (view-major)
__global__ __launch_bounds__(FUSE_SCAN) void fuse_scan_kernel(const FuseParams F) {
  __shared__ int wt[FUSE_SCAN_WAVES];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nblk = F.V * F.nb, per = (nblk + FUSE_SCAN - 1) / FUSE_SCAN;
  int* bs = F.bsum + (long)b * nblk;
  const int lo = std::min(t * per, nblk), hi = std::min(lo + per, nblk);
  int mine = 0;
#pragma unroll 1
  for (int i = lo; i < hi; ++i) mine += bs[i];
  int sum;
  int before = wg_scan_exclusive<FUSE_SCAN_WAVES>(mine, wt, sum);
#pragma unroll 1
  for (int i = lo; i < hi; ++i) {
    const int cnt = bs[i];
    bs[i] = before;
    before += cnt;
  }
  if (t == 0) {
    const int emitted = std::min(sum, F.max_points);
    F.total[b] = sum;
    F.counts[b] = emitted;
    F.stats[(long)b * FUSE_STATS + 4] = emitted;
  }
}

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_emit_kernel(const FuseParams F, const FuseColors C) {
  __shared__ FView sv[FUSE_MAX_VIEWS];
  __shared__ int wcnt[FUSE_WAVES];
  const int v = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
  fuse_stage_views(F, b, sv);
  const int n = F.H * F.W, q = blockIdx.x * FUSE_BLOCK + t;
  const bool in = q < n;
  const long at = ((long)b * F.V + v) * n + q;
  const bool emit = in && F.state[at] == 1;
  const int blk = v * F.nb + blockIdx.x;
  const int before = F.bsum[(long)b * F.V * F.nb + blk];  // emitted by the earlier blocks; the load flies during the rank's barrier
  int emitted;  // of the block: not needed
  const int in_block = wg_rank<FUSE_WAVES>(emit, wcnt, emitted);
  const float nanf_ = __int_as_float(0x7fc00000);
  const long cloud = (long)b * F.max_points;
  if (emit) {
    const int rank = before + in_block;
    if (rank < F.max_points) {
      const int r = q / F.W, c = q - r * F.W;
      double X[3];
      fuse_world(sv[v], r, c, (double)F.depth[at], X);
      float* xyz = F.out_points + (cloud + rank) * 3;
      xyz[0] = (float)X[0], xyz[1] = (float)X[1], xyz[2] = (float)X[2];
      F.out_weight[cloud + rank] = F.weight[at];
      F.out_source[(cloud + rank) * 2 + 0] = v;
      F.out_source[(cloud + rank) * 2 + 1] = q;
      if (F.out_colors) {
        // the image pixel that holds the centre of the cell: floor((c + 0.5) W_img / W) in integers
        const int cv = b * F.V + v;
        const long ix = ((2l * c + 1) * C.w[cv]) / (2l * F.W), iy = ((2l * r + 1) * C.h[cv]) / (2l * F.H);
        const unsigned char* px = C.images + C.offset[cv] + (iy * C.w[cv] + ix) * 3;
        unsigned char* rgb = F.out_colors + (cloud + rank) * 3;
        rgb[0] = px[0], rgb[1] = px[1], rgb[2] = px[2];
      }
    }
  }
  // the padding beyond the cloud, by the threads of the whole problem
  const long first = std::min(F.total[b], F.max_points), step = (long)F.V * F.nb * FUSE_BLOCK;
#pragma unroll 1
  for (long i = first + (long)blk * FUSE_BLOCK + t; i < F.max_points; i += step) {
    float* xyz = F.out_points + (cloud + i) * 3;
    xyz[0] = nanf_, xyz[1] = nanf_, xyz[2] = nanf_;
    F.out_weight[cloud + i] = 0.0f;
    F.out_source[(cloud + i) * 2 + 0] = -1;
    F.out_source[(cloud + i) * 2 + 1] = -1;
    if (F.out_colors) {
      unsigned char* rgb = F.out_colors + (cloud + i) * 3;
      rgb[0] = 0, rgb[1] = 0, rgb[2] = 0;
    }
  }
}

struct RelParams {
  const double* R;
  const double* t;
  int B, V, P;
  double* out_R;
  double* out_t;
  unsigned char pv[FUSE_MAX_PAIRS][2];
};

// R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i: one thread per (problem, pair)
__global__ __launch_bounds__(64) void relative_poses_kernel(const RelParams Q) {
  const long k = (long)blockIdx.x * 64 + threadIdx.x;
  if (k >= (long)Q.B * Q.P) return;
  const int b = (int)(k / Q.P), p = (int)(k - (long)b * Q.P);
  const int i = Q.pv[p][0], j = Q.pv[p][1];
  const double* Ri = Q.R + ((long)b * Q.V + i) * 9;
  const double* Rj = Q.R + ((long)b * Q.V + j) * 9;
  const double* ti = Q.t + ((long)b * Q.V + i) * 3;
  const double* tj = Q.t + ((long)b * Q.V + j) * 3;
  double* Ro = Q.out_R + k * 9;
  double* to = Q.out_t + k * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double row[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c] = (Rj[a * 3 + 0] * Ri[c * 3 + 0] + Rj[a * 3 + 1] * Ri[c * 3 + 1]) + Rj[a * 3 + 2] * Ri[c * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) Ro[a * 3 + c] = row[c];
    to[a] = tj[a] - ((row[0] * ti[0] + row[1] * ti[1]) + row[2] * ti[2]);
  }
}

// the workspace regions of F; returns the bytes of the workspace
size_t fuse_carve(Workspace256 ws, int B, int V, int H, int W, FuseParams& F) {
  const long n = (long)H * W, nb = (n + FUSE_BLOCK - 1) / FUSE_BLOCK;
  F.keep = ws.take<unsigned char>((size_t)B * V * n);
  F.bsum = ws.take<int>((size_t)B * V * nb);
  return ws.bytes();
}

bool fuse_sizes_ok(int B, int V, int H, int W) {
  return B >= 1 && B <= 65535 && V >= 2 && V <= FUSE_MAX_VIEWS && H >= 1 && W >= 1 && W <= (1 << 30) &&
         (long)H * W < (1l << 31) / ((long)B * V);
}

}  // namespace

extern "C" long roma_op_fuse_depth_maps_workspace(int B, int V, int H, int W) {
  if (!fuse_sizes_ok(B, V, H, W)) return 0;
  FuseParams F;
  return fuse_carve(Workspace256(), B, V, H, W, F);
}

extern "C" int roma_op_fuse_depth_maps(const float* points, const unsigned char* flags, const float* certainty, const int* pair_views,
                                       const double* cameras, const double* R, const double* t, const unsigned char* view_valid,
                                       const unsigned char* valid, const unsigned char* images, const long long* image_offsets,
                                       const int* image_sizes, int B, int V, int P, int H, int W, int symmetric, double rel_thresh,
                                       int min_support, int min_consistent, int max_violations, int dedupe, int max_points,
                                       float* out_depth, float* out_weight, unsigned char* out_support, unsigned char* out_seen,
                                       unsigned char* out_violated, unsigned char* out_state, float* out_points, unsigned char* out_colors,
                                       float* out_cloud_weight, int* out_source, int* out_counts, int* out_total, int* out_stats, void* ws,
                                       long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(points && flags && pair_views && cameras && R && t, "fuse_depth_maps: null pointer");
  ROMA_REQUIRE(out_depth && out_weight && out_support && out_seen && out_violated && out_state && out_points && out_cloud_weight &&
                   out_source && out_counts && out_total && out_stats,
               "fuse_depth_maps: null pointer");
  ROMA_REQUIRE(V >= 2 && V <= FUSE_MAX_VIEWS, "fuse_depth_maps: need 2 <= V <= 8 views");
  ROMA_REQUIRE(P >= 1 && P <= FUSE_MAX_PAIRS, "fuse_depth_maps: need 1 <= P <= 64 pairs");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "fuse_depth_maps: B must lie in [0, 65535]");
  ROMA_REQUIRE(H >= 1 && W >= 1, "fuse_depth_maps: H and W must be positive");
  ROMA_REQUIRE(symmetric == 0 || symmetric == 1, "fuse_depth_maps: symmetric must be 0 or 1");
  ROMA_REQUIRE(dedupe == 0 || dedupe == 1, "fuse_depth_maps: dedupe must be 0 or 1");
  ROMA_REQUIRE(rel_thresh >= 0, "fuse_depth_maps: rel_thresh is negative (or NaN)");
  ROMA_REQUIRE(min_support >= 1 && min_support <= FUSE_MAX_SLOTS, "fuse_depth_maps: need 1 <= min_support <= 14");
  ROMA_REQUIRE(min_consistent >= 0 && min_consistent <= FUSE_MAX_VIEWS - 1, "fuse_depth_maps: need 0 <= min_consistent <= 7");
  ROMA_REQUIRE(max_violations >= 0, "fuse_depth_maps: max_violations must not be negative");
  ROMA_REQUIRE(max_points >= 0, "fuse_depth_maps: max_points must not be negative");
  FuseParams F = {};
  if (int rc = check_pairs("fuse_depth_maps", pair_views, V, P, F.pv)) return rc;
  for (int p = 0; p < P; ++p)
    for (int k = 0; k < p; ++k)
      ROMA_REQUIRE(F.pv[p][0] != F.pv[k][0] || F.pv[p][1] != F.pv[k][1], "fuse_depth_maps: pair_views holds an ordered pair twice");
  ROMA_REQUIRE((images != nullptr) == (image_offsets != nullptr) && (images != nullptr) == (image_sizes != nullptr),
               "fuse_depth_maps: images, image_offsets and image_sizes go together");
  ROMA_REQUIRE(!out_colors || images, "fuse_depth_maps: out_colors needs the colour source");
  if (B == 0) return 0;
  const int Wd = symmetric ? 2 * W : W;
  ROMA_REQUIRE(W <= (1 << 30) && (long)H * Wd < (1l << 31) / ((long)B * P) && (long)H * W < (1l << 31) / ((long)B * V),
               "fuse_depth_maps: B * P * H * Wd and B * V * H * W must be below 2^31");
  ROMA_REQUIRE((long)max_points < (1l << 31) / (3l * B), "fuse_depth_maps: 3 * B * max_points must be below 2^31");
  FuseColors C = {};
  if (out_colors) {
    ROMA_REQUIRE(B * V <= FUSE_MAX_COLOR_VIEWS, "fuse_depth_maps: with a colour source B * V must not exceed 128");
    for (int k = 0; k < B * V; ++k) {
      ROMA_REQUIRE(image_sizes[2 * k] >= 1 && image_sizes[2 * k + 1] >= 1 && image_offsets[k] >= 0,
                   "fuse_depth_maps: image sizes must be positive and image offsets not negative");
      C.offset[k] = image_offsets[k], C.h[k] = image_sizes[2 * k], C.w[k] = image_sizes[2 * k + 1];
    }
    C.images = images;
  }
  ROMA_REQUIRE(ws && ws_bytes >= (size_t)roma_op_fuse_depth_maps_workspace(B, V, H, W), "fuse_depth_maps: workspace too small");
  // the slots of every view: the halves on its grid, in ascending pair
  for (int p = 0; p < P; ++p)
    for (int half = 0; half < (symmetric ? 2 : 1); ++half) {
      const int v = F.pv[p][half];
      F.slot[v][F.nslots[v]++] = (unsigned char)(p * 2 + half);  // at most 2 (V - 1): no ordered pair occurs twice
    }
  fuse_carve(Workspace256(ws), B, V, H, W, F);
  F.points = points, F.flags = flags, F.cert = certainty, F.cam = cameras, F.R = R, F.t = t, F.view_valid = view_valid, F.valid = valid;
  F.B = B, F.V = V, F.P = P, F.H = H, F.W = W, F.Wd = Wd;
  F.rel = rel_thresh;
  F.min_support = min_support, F.min_consistent = min_consistent, F.max_violations = max_violations, F.dedupe = dedupe;
  F.max_points = max_points;
  F.depth = out_depth, F.weight = out_weight, F.support = out_support, F.seen = out_seen, F.violated = out_violated, F.state = out_state;
  F.out_points = out_points, F.out_colors = out_colors, F.out_weight = out_cloud_weight, F.out_source = out_source;
  F.counts = out_counts, F.total = out_total, F.stats = out_stats;
  const long n = (long)H * W;
  F.nb = (int)((n + FUSE_BLOCK - 1) / FUSE_BLOCK);
  ROMA_CHECK_HIP(hipMemsetAsync(out_stats, 0, (size_t)B * FUSE_STATS * sizeof(int), s));
  const dim3 grid(F.nb, V, B);
  const double px = (double)B * V * (double)n;
  {
    int slots = 0;
    for (int v = 0; v < V; ++v) slots += F.nslots[v];
    // the bytes the vote must read: depth, flag and certainty of every slot, and the three maps it writes
    ProfScope ps("fuse_select_kernel", (double)B * (double)n * (slots * (certainty ? 9.0 : 5.0) + V * 9.0), "B", s);
    hipLaunchKernelGGL(fuse_select_kernel, grid, dim3(FUSE_BLOCK), 0, s, F);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("fuse_check_kernel", px * 7.0, "B", s);
    hipLaunchKernelGGL(fuse_check_kernel, grid, dim3(FUSE_BLOCK), 0, s, F);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("fuse_dedupe_kernel", px * 7.0, "B", s);
    hipLaunchKernelGGL(fuse_dedupe_kernel, grid, dim3(FUSE_BLOCK), 0, s, F);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("fuse_scan_kernel", (double)B * V * F.nb * 8.0, "B", s);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(B), dim3(FUSE_SCAN), 0, s, F);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("fuse_emit_kernel", px * 1.0 + (double)B * max_points * 27.0, "B", s);
    hipLaunchKernelGGL(fuse_emit_kernel, grid, dim3(FUSE_BLOCK), 0, s, F, C);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int roma_op_relative_poses(const double* R, const double* t, const int* pair_views, int B, int V, int P, double* out_R,
                                      double* out_t, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(R && t && pair_views && out_R && out_t, "relative_poses: null pointer");
  ROMA_REQUIRE(V >= 2 && V <= FUSE_MAX_VIEWS, "relative_poses: need 2 <= V <= 8 views");
  ROMA_REQUIRE(P >= 1 && P <= FUSE_MAX_PAIRS, "relative_poses: need 1 <= P <= 64 pairs");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "relative_poses: B must lie in [0, 65535]");
  RelParams Q = {};
  if (int rc = check_pairs("relative_poses", pair_views, V, P, Q.pv)) return rc;
  if (B == 0) return 0;
  Q.R = R, Q.t = t, Q.B = B, Q.V = V, Q.P = P, Q.out_R = out_R, Q.out_t = out_t;
  ProfScope ps("relative_poses_kernel", (double)B * P * 96.0, "B", s);
  hipLaunchKernelGGL(relative_poses_kernel, dim3((unsigned)(((long)B * P + 63) / 64)), dim3(64), 0, s, Q);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
