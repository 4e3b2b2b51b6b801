// Point-cloud rendering (roma_op_render_points): the N rows of a world-space point cloud - DenseFusion.points as it is, NaN padding
// included - are splatted into C cameras per problem with a z-buffer, back-surface points that show through the gaps of a nearer
// surface are removed, small holes are closed, and depth, row index, colour and a mask come out per pixel.  The definition is in
// include/roma_hip.h; tools/point_render_ref.py restates it in numpy float64, operation by operation, and is the oracle of
// tests/test_gpu_point_render.py.
//
// The z-buffer holds one 64-bit key per pixel, (bits of the float32 depth) << 32 | row: the depth is positive, so the integer order
// of its bits is its numeric order, and the minimum of the keys offered to a pixel is the nearest depth, then the lowest row -
// whatever the order of arrival.  Four steps on the stream, every phase closed by a kernel boundary - what one kernel decides is
// read only by the next:
//   clear    the key buffer to all ones ("empty") and stats to 0, two memsets: the workspace need not be clear on entry
//   splat    grid (blocks of 256 rows, camera, problem): the camera is the same for a whole workgroup and staged once in LDS; the
//            point is loaded once, widened and projected in float64; its key goes to the (2 radius + 1)^2 pixels around its cell
//            by a 64-bit atomicMin.  A key only ever decreases, so a plain load first - `if (key < seen) atomicMin` - is exact:
//            a stale value is a larger one and can only cost an atomic that was not needed, never skip one that was
//   filter   one thread per pixel, reads the raw keys only: a hit pixel is removed when occlusion_count hit pixels of its window
//            are nearer by more than occlusion_rel; one decision byte per pixel
//   fill     one thread per pixel, reads the decision bytes and the keys of the survivors: an empty or removed pixel with fill_min
//            survivors in its window takes the smallest of their keys; then every output of the pixel is written
// The only other atomics are the integer counters of `stats`, one per workgroup that has something to count.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "common.h"
#include "workgroup.h"
#include "workspace.h"

// nothing here is fused: tools/point_render_ref.py evaluates the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

typedef unsigned long long u64;

constexpr int RENDER_MAX_RADIUS = 4;  // splat, occlusion and fill windows: at most 9 x 9
constexpr int RENDER_STATS = 4;       // ints per frame in roma_op_render_points' out_stats
constexpr int RND_BLOCK = 256, RND_WAVES = RND_BLOCK / WAVE;
constexpr u64 RND_EMPTY = ~0ull;

struct RenderParams {
  const float* points;
  const unsigned char* colors;
  const int* counts;
  const unsigned char* valid;
  const double* cam;
  const double* R;
  const double* t;
  int B, N, C, H, W;
  int radius, occ_radius, occ_count, fill_radius, fill_min;
  double near, far, occ_factor;  // occ_factor = 1.0 + occlusion_rel
  unsigned char bg[3];
  unsigned char* color;
  float* depth;
  int* index;
  unsigned char* mask;
  int* stats;
  u64* key;            // [B, C, H, W] workspace: the z-buffer
  unsigned char* dec;  // [B, C, H, W] workspace: bit 0 hit, bit 1 removed
};

__device__ __forceinline__ float render_key_depth(u64 key) { return __uint_as_float((unsigned)(key >> 32)); }

__global__ __launch_bounds__(RND_BLOCK) void render_splat_kernel(const RenderParams P) {
  __shared__ double sc[16];  // the camera of the workgroup, once: R, t, then fx, fy, cx, cy
  __shared__ int wc[RND_WAVES];
  const int k = blockIdx.y, b = blockIdx.z;
  const long frame = (long)b * P.C + k;
  if (threadIdx.x < 16) {
    const int i = threadIdx.x;
    const int ci = i == 12 ? 0 : i == 13 ? 4 : i == 14 ? 2 : 5;
    sc[i] = i < 9 ? P.R[frame * 9 + i] : i < 12 ? P.t[frame * 3 + (i - 9)] : P.cam[frame * 9 + ci];
  }
  __syncthreads();
  const bool on = !P.valid || P.valid[b] != 0;
  int cnt = P.N;  // min(max(counts[b], 0), N), by value: std::min on a loaded int takes its address and costs scratch here
  if (P.counts) {
    const int given = P.counts[b];
    cnt = given < 0 ? 0 : given < P.N ? given : P.N;
  }
  const long n = (long)blockIdx.x * RND_BLOCK + threadIdx.x;
  bool usable = false;
  int r0 = 0, c0 = 0;
  u64 key = RND_EMPTY;
  if (on && n < cnt) {
    const float* p = P.points + ((long)b * P.N + n) * 3;
    const float x0 = p[0], x1 = p[1], x2 = p[2];
    if (isfinite(x0) && isfinite(x1) && isfinite(x2)) {
      const double X0 = (double)x0, X1 = (double)x1, X2 = (double)x2;
      const double yx = ((sc[0] * X0 + sc[1] * X1) + sc[2] * X2) + sc[9];
      const double yy = ((sc[3] * X0 + sc[4] * X1) + sc[5] * X2) + sc[10];
      const double yz = ((sc[6] * X0 + sc[7] * X1) + sc[8] * X2) + sc[11];
      if (yz >= P.near && yz <= P.far) {  // NaN fails
        const float zf = (float)yz;
        const double u = sc[12] * (yx / yz) + sc[14], v = sc[13] * (yy / yz) + sc[15];
        if (isfinite(zf) && zf > 0.0f && isfinite(u) && isfinite(v)) {
          // in or out of reach is decided in double, before any conversion to an integer
          const double fu = floor(u), fv = floor(v), rad = (double)P.radius;
          if (fu >= -rad && fu < (double)P.W + rad && fv >= -rad && fv < (double)P.H + rad) {
            usable = true;
            c0 = (int)fu, r0 = (int)fv;
            key = ((u64)__float_as_uint(zf) << 32) | (u64)(unsigned)n;
          }
        }
      }
    }
  }
  if (usable) {
    u64* K = P.key + frame * ((long)P.H * P.W);
#pragma unroll 1
    for (int dr = -P.radius; dr <= P.radius; ++dr) {
      const int r = r0 + dr;
      if (r < 0 || r >= P.H) continue;
#pragma unroll 1
      for (int dc = -P.radius; dc <= P.radius; ++dc) {
        const int c = c0 + dc;
        if (c < 0 || c >= P.W) continue;
        u64* q = K + ((long)r * P.W + c);
#ifndef ROMA_RENDER_NO_EARLY_OUT  // the A/B build of tools/bench_point_render.py: every offer is an atomic
        if (key < __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
#endif
          atomicMin(q, key);
      }
    }
  }
  wg_count_add<RND_WAVES>(P.stats + frame * RENDER_STATS + 0, usable && r0 >= 0 && r0 < P.H && c0 >= 0 && c0 < P.W, wc);
}

__global__ __launch_bounds__(RND_BLOCK) void render_filter_kernel(const RenderParams P) {
  __shared__ int wc[RND_WAVES];
  const long frame = (long)blockIdx.z * P.C + blockIdx.y;
  const int npx = P.H * P.W, q = blockIdx.x * RND_BLOCK + threadIdx.x;
  const bool in = q < npx;
  const u64* K = P.key + frame * npx;
  const u64 key = in ? K[q] : RND_EMPTY;
  const bool hit = key != RND_EMPTY;
  bool removed = false;
  if (hit && P.occ_radius > 0) {
    const int r = q / P.W, c = q - r * P.W;
    const double z = (double)render_key_depth(key);
    const int ra = std::max(r - P.occ_radius, 0), rb = std::min(r + P.occ_radius, P.H - 1);
    const int ca = std::max(c - P.occ_radius, 0), cb = std::min(c + P.occ_radius, P.W - 1);
    int nearer = 0;
#pragma unroll 1
    for (int rr = ra; rr <= rb; ++rr)
#pragma unroll 1
      for (int cc = ca; cc <= cb; ++cc) {
        const u64 kq = K[(long)rr * P.W + cc];
        if (kq != RND_EMPTY && z > (double)render_key_depth(kq) * P.occ_factor) ++nearer;
      }
    removed = nearer >= P.occ_count;
  }
  int* stats = P.stats + frame * RENDER_STATS;
  wg_count_add<RND_WAVES>(stats + 1, hit, wc);
  wg_count_add<RND_WAVES>(stats + 2, removed, wc);
  if (in) P.dec[frame * npx + q] = (unsigned char)((hit ? 1 : 0) | (removed ? 2 : 0));
}

__global__ __launch_bounds__(RND_BLOCK) void render_fill_kernel(const RenderParams P) {
  __shared__ int wc[RND_WAVES];
  const int b = blockIdx.z;
  const long frame = (long)b * P.C + blockIdx.y;
  const int npx = P.H * P.W, q = blockIdx.x * RND_BLOCK + threadIdx.x;
  const bool in = q < npx;
  const u64* K = P.key + frame * npx;
  const unsigned char* D = P.dec + frame * npx;
  const unsigned d = in ? D[q] : 0u;
  u64 key = d == 1u ? K[q] : RND_EMPTY;  // a survivor keeps its key
  bool filled = false;
  if (in && d != 1u && P.fill_radius > 0) {
    const int r = q / P.W, c = q - r * P.W;
    const int ra = std::max(r - P.fill_radius, 0), rb = std::min(r + P.fill_radius, P.H - 1);
    const int ca = std::max(c - P.fill_radius, 0), cb = std::min(c + P.fill_radius, P.W - 1);
    int alive = 0;
    u64 best = RND_EMPTY;
#pragma unroll 1
    for (int rr = ra; rr <= rb; ++rr)
#pragma unroll 1
      for (int cc = ca; cc <= cb; ++cc) {
        const long at = (long)rr * P.W + cc;
        if (D[at] == 1) {
          ++alive;
          best = std::min(best, K[at]);
        }
      }
    filled = alive >= P.fill_min;
    if (filled) key = best;
  }
  wg_count_add<RND_WAVES>(P.stats + frame * RENDER_STATS + 3, filled, wc);
  if (!in) return;
  const long at = frame * npx + q;
  const bool have = key != RND_EMPTY;
  const int row = (int)(unsigned)(key & 0xFFFFFFFFull);
  P.depth[at] = have ? render_key_depth(key) : __int_as_float(0x7fc00000);
  P.index[at] = have ? row : -1;
  P.mask[at] = (unsigned char)(d | (filled ? 4u : 0u));
  if (P.color) {
    unsigned char* rgb = P.color + at * 3;
    if (have) {
      const unsigned char* px = P.colors + ((long)b * P.N + row) * 3;
      rgb[0] = px[0], rgb[1] = px[1], rgb[2] = px[2];
    } else {
      rgb[0] = P.bg[0], rgb[1] = P.bg[1], rgb[2] = P.bg[2];
    }
  }
}

// 3 B C H W < 2^31, by a division: the product itself may not fit
bool render_pixels_ok(int B, int C, int H, int W) { return (long)H * W <= ((1l << 31) - 1) / (3l * B * C); }

bool render_sizes_ok(int B, int C, int H, int W) {
  return B >= 1 && C >= 1 && (long)B * C <= 65535 && H >= 1 && W >= 1 && render_pixels_ok(B, C, H, W);
}

// the workspace regions of P, one entry per pixel each; returns the bytes of the workspace
size_t render_carve(Workspace256 ws, size_t npx, RenderParams& P) {
  P.key = ws.take<u64>(npx);
  P.dec = ws.take<unsigned char>(npx);
  return ws.bytes();
}

}  // namespace

extern "C" long roma_op_render_points_workspace(int B, int C, int H, int W) {
  if (!render_sizes_ok(B, C, H, W)) return 0;
  RenderParams P;
  return render_carve(Workspace256(), (size_t)B * C * H * W, P);
}

extern "C" int roma_op_render_points(const float* points, const unsigned char* colors, const int* counts, const unsigned char* valid,
                                     const double* cameras, const double* R, const double* t, int B, int N, int C, int H, int W, int radius,
                                     double near, double far, int occlusion_radius, double occlusion_rel, int occlusion_count,
                                     int fill_radius, int fill_min, int background, unsigned char* out_color, float* out_depth,
                                     int* out_index, unsigned char* out_mask, int* out_stats, void* ws, long workspace_bytes,
                                     void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(points && cameras && R && t, "render_points: null pointer");
  ROMA_REQUIRE(out_depth && out_index && out_mask && out_stats, "render_points: null pointer");
  ROMA_REQUIRE((colors != nullptr) == (out_color != nullptr), "render_points: colors and out_color go together");
  ROMA_REQUIRE(C >= 1, "render_points: need C >= 1 cameras");
  ROMA_REQUIRE(B >= 0 && (long)B * C <= 65535, "render_points: B must not be negative and B * C must not exceed 65535");
  ROMA_REQUIRE(H >= 1 && W >= 1, "render_points: H and W must be positive");
  ROMA_REQUIRE(N >= 0, "render_points: N must not be negative");
  ROMA_REQUIRE(radius >= 0 && radius <= RENDER_MAX_RADIUS && occlusion_radius >= 0 && occlusion_radius <= RENDER_MAX_RADIUS &&
                   fill_radius >= 0 && fill_radius <= RENDER_MAX_RADIUS,
               "render_points: radius, occlusion_radius and fill_radius must lie in [0, 4]");
  ROMA_REQUIRE(occlusion_count >= 1 && fill_min >= 1, "render_points: occlusion_count and fill_min must be at least 1");
  ROMA_REQUIRE(occlusion_rel >= 0, "render_points: occlusion_rel is negative (or NaN)");
  ROMA_REQUIRE(near > 0, "render_points: near must be positive");
  ROMA_REQUIRE(far >= near, "render_points: far is below near (or NaN)");
  ROMA_REQUIRE(background >= 0 && background <= 0xFFFFFF, "render_points: background is r | g << 8 | b << 16");
  if (B == 0) return 0;
  ROMA_REQUIRE(render_pixels_ok(B, C, H, W), "render_points: 3 * B * C * H * W must be below 2^31");
  ROMA_REQUIRE(ws && ws_bytes >= (size_t)roma_op_render_points_workspace(B, C, H, W), "render_points: workspace too small");
  RenderParams P = {};
  const size_t npx = (size_t)B * C * H * W;
  render_carve(Workspace256(ws), npx, P);
  P.points = points, P.colors = colors, P.counts = counts, P.valid = valid, P.cam = cameras, P.R = R, P.t = t;
  P.B = B, P.N = N, P.C = C, P.H = H, P.W = W;
  P.radius = radius, P.occ_radius = occlusion_radius, P.occ_count = occlusion_count, P.fill_radius = fill_radius, P.fill_min = fill_min;
  P.near = near, P.far = far, P.occ_factor = 1.0 + occlusion_rel;
  P.bg[0] = (unsigned char)(background & 255), P.bg[1] = (unsigned char)((background >> 8) & 255);
  P.bg[2] = (unsigned char)((background >> 16) & 255);
  P.color = out_color, P.depth = out_depth, P.index = out_index, P.mask = out_mask, P.stats = out_stats;
  const double px = (double)npx, splat = (2.0 * radius + 1.0) * (2.0 * radius + 1.0);
  {
    ProfScope ps("render_clear", px * 8.0, "B", s);
    ROMA_CHECK_HIP(hipMemsetAsync(out_stats, 0, (size_t)B * C * RENDER_STATS * sizeof(int), s));
    ROMA_CHECK_HIP(hipMemsetAsync(P.key, 0xFF, npx * sizeof(u64), s));
  }
  if (N > 0) {
    // the keys a frame is offered when every row is usable and no splat is clipped: the unit is 8-byte offers, not bytes moved
    ProfScope ps("render_splat_kernel", (double)B * C * (double)N * splat, "offers", s);
    hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)(((long)N + RND_BLOCK - 1) / RND_BLOCK), C, B), dim3(RND_BLOCK), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  const dim3 grid((unsigned)(((long)H * W + RND_BLOCK - 1) / RND_BLOCK), C, B);
  {
    ProfScope ps("render_filter_kernel", px * 9.0, "B", s);
    hipLaunchKernelGGL(render_filter_kernel, grid, dim3(RND_BLOCK), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("render_fill_kernel", px * (9.0 + 9.0 + (colors ? 6.0 : 0.0)), "B", s);
    hipLaunchKernelGGL(render_fill_kernel, grid, dim3(RND_BLOCK), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace roma
