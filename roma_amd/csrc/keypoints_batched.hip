// RegressionMatcher.match_keypoints (romatch/models/matcher.py:732-773) for B pairs in one enqueue: per pair b with
// na = counts_a[b], nb = counts_b[b] rows, the mutual nearest neighbours between the warped keypoints of A and the keypoints of B,
// every tied pair, row-major, padded to M rows and counted (roma_op_match_keypoints in include/roma_hip.h states the definition,
// tools/keypoints_ref.py restates it in numpy float32).  The single-pair route (keypoints.hip) reads its pair count back between
// two calls; here nothing is read back and nothing is allocated, so the result feeds the batched geometry through `counts`.
//
// Five launches on the caller's stream whatever B is, the pair is the last grid axis of each:
//   1. kp_sample_kernel   p_i, c_i = bilinear(warp[b][..., 2:4], certainty[b]) at x_A[b, i] - sample_warp_at_kernel's expression,
//                         term for term - and the row / column minima set to "nothing seen";
//   2. kp_nn_kernel       both directions in one grid (x = A-blocks then B-blocks, y = slices of the scanned side): the minimum
//                         of d2 = fmaf(dy, dy, dx * dx) over the scanned points, staged in LDS tiles of 1024 and read as wave-wide
//                         broadcasts; slices merge by an integer atomicMin on the bits of d2 (d2 >= 0: integer order is numeric
//                         order), which gives the same word in any order.  Only the minimum is kept, no index: the pairs are
//                         found again below from the bits of both minima, which is what makes every tie come out;
//   3. kp_pairs_kernel<0> per A row and slice of B the number of j with bits(d2(i, j)) == row minimum == column minimum (rows
//                         that fail the certainty or the distance test count nothing, a workgroup without a live row leaves
//                         before its first tile);
//   4. kp_scan_kernel     one workgroup per pair: exclusive 64-bit prefix sums over (row, slice) in that order = row-major
//                         positions; total[b], counts[b] = min(total, M), and the rows at and beyond counts[b] set to -1 / 0;
//   5. kp_pairs_kernel<1> the same walk as 3, writing pair number k < M of the pair to inds / kpts_a / kpts_b.
// No output position comes from an atomic, no float is added: a pair's result is a function of its own rows alone, whatever B,
// its place in the batch, or the padding widths NA / NB (which only move the slice boundaries of commutative minima and of
// counts that are added up in order).  A workgroup whose block of rows or slice lies beyond the pair's counts exits before
// its first load of point data; rows at or beyond the counts are never read.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "common.h"
#include "workgroup.h"
#include "workspace.h"

namespace roma {
namespace {

constexpr int KP_THREADS = 256;
constexpr int KP_TILE = 1024;          // scanned points per LDS tile
constexpr int KP_COUNT_SLICES = 8;     // at most this many slices of B in the count / fill walk
constexpr long KP_MAX_POINTS = 1l << 20;
constexpr long KP_TARGET_GROUPS = 1024;  // 4 workgroups of 256 on each of 256 CUs
constexpr unsigned KP_NONE = 0xffffffffu;  // as a float a NaN: below no threshold

struct KpParams {
  const float* xa;  // [B, NA, 2]
  const float* xb;  // [B, NB, 2]
  const int* counts_a;
  const int* counts_b;
  const float* warp;
  long warp_bs, warp_rs;  // floats
  const float* cert;
  long cert_bs, cert_rs;  // floats
  const float* sizes;     // [B, 4] (H_A, W_A, H_B, W_B) or null
  long sizes_bs;
  long NA, NB, M;
  int H, W;
  float cert_th, max_d2;
  int blocks_a;             // workgroups over the A rows (at least 1)
  long nn_per_a, nn_per_b;  // scanned points of A / of B per slice of kp_nn_kernel (multiples of KP_TILE)
  int cnt_slices;           // slices of B in kp_pairs_kernel
  long cnt_per;             // points of B per such slice (a multiple of KP_TILE)
  float* p;                 // [B, NA, 2]  warped keypoints of A
  float* c;                 // [B, NA]     their certainty
  unsigned* min_a;          // [B, NA]     bits of the row minimum
  unsigned* min_b;          // [B, NB]     bits of the column minimum
  long long* offs;          // [B, NA, cnt_slices]  counts, then exclusive prefix sums
  int* inds;
  float* kpts_a;
  float* kpts_b;
  int* counts;
  long long* total;
};

__device__ __forceinline__ long pair_rows(const int* counts, int b, long N) {
  return counts ? min((long)max(counts[b], 0), N) : N;
}

// ------------------------------------------------------------------ 1. sample; grid (max(A-blocks, B-blocks), B)
__global__ __launch_bounds__(KP_THREADS) void kp_sample_kernel(const KpParams A) {
  const int b = blockIdx.y;
  const long na = pair_rows(A.counts_a, b, A.NA), nb = pair_rows(A.counts_b, b, A.NB);
  const long i = (long)blockIdx.x * KP_THREADS + threadIdx.x;
  if (i < nb) A.min_b[(long)b * A.NB + i] = KP_NONE;
  if (i >= na) return;
  const float* xa = A.xa + (long)b * A.NA * 2;
  const float* warp = A.warp + (long)b * A.warp_bs;
  const float* cert = A.cert + (long)b * A.cert_bs;
  const int H = A.H, W = A.W;
  // sample_warp_at_kernel (keypoints.hip), term for term
  const float gx = xa[i * 2 + 0], gy = xa[i * 2 + 1];
  float ix = ((gx + 1.f) * W - 1.f) * 0.5f, iy = ((gy + 1.f) * H - 1.f) * 0.5f;  // align_corners=False
  ix = fminf(fmaxf(ix, -1.0e6f), 1.0e6f);
  iy = fminf(fmaxf(iy, -1.0e6f), 1.0e6f);
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float tx = ix - fx0, ty = iy - fy0;
  const float wgt[4] = {(1.f - tx) * (1.f - ty), tx * (1.f - ty), (1.f - tx) * ty, tx * ty};
  float bx = 0.f, by = 0.f, c = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {  // zeros padding
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(warp + (long)yy * A.warp_rs + 4l * xx);
      bx += wgt[t] * w4[2];
      by += wgt[t] * w4[3];
      c += wgt[t] * cert[(long)yy * A.cert_rs + xx];
    }
  }
  const long o = (long)b * A.NA + i;
  A.p[o * 2 + 0] = bx;
  A.p[o * 2 + 1] = by;
  A.c[o] = c;
  A.min_a[o] = KP_NONE;
}

// ------------------------------------------------------------------ 2. both nearest-neighbour passes
// grid (A-blocks + B-blocks, slices, B).  A block of 256 points p keeps the minimum squared distance to its slice of the other
// side's points q; per distance two subtractions, a multiply, a fused multiply-add and (a share of) a minimum on two broadcast
// LDS floats.  A NaN distance is ignored, as `d2 < best` in nn_kernel ignores it.
__global__ __launch_bounds__(KP_THREADS) void kp_nn_kernel(const KpParams A) {
  __shared__ __attribute__((aligned(16))) float qs[KP_TILE * 2];
  const int b = blockIdx.z;
  const long na = pair_rows(A.counts_a, b, A.NA), nb = pair_rows(A.counts_b, b, A.NB);
  const bool rev = (int)blockIdx.x >= A.blocks_a;  // points of B against the warped points of A
  const long blk = rev ? (long)blockIdx.x - A.blocks_a : (long)blockIdx.x;
  const long np = rev ? nb : na, nq = rev ? na : nb;
  const long per = rev ? A.nn_per_a : A.nn_per_b;
  const long j_begin = (long)blockIdx.y * per;
  if (blk * KP_THREADS >= np || j_begin >= nq) return;
  const long j_end = min(nq, j_begin + per);
  const float* pa = A.p + (long)b * A.NA * 2;
  const float* pb = A.xb + (long)b * A.NB * 2;
  const float* p = rev ? pb : pa;
  const float* q = rev ? pa : pb;
  const long i = blk * KP_THREADS + threadIdx.x;
  float px = 0.f, py = 0.f;
  if (i < np) {
    px = p[i * 2 + 0];
    py = p[i * 2 + 1];
  }
  float bd = INFINITY;
  for (long j0 = j_begin; j0 < j_end; j0 += KP_TILE) {
    const int cnt = (int)min((long)KP_TILE, j_end - j0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * 2; t += KP_THREADS) qs[t] = q[j0 * 2 + t];
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < cnt; ++t) {
      const float dx = px - qs[2 * t], dy = py - qs[2 * t + 1];
      bd = fminf(bd, fmaf(dy, dy, dx * dx));  // the expression of nn_kernel
    }
  }
  if (i < np) atomicMin((rev ? A.min_b + (long)b * A.NB : A.min_a + (long)b * A.NA) + i, __float_as_uint(bd));
}

// ------------------------------------------------------------------ 3. and 5. the pairs of every row, counted (MODE 0) or written
// grid (A-blocks, cnt_slices, B).  Entry (i, s) of offs: MODE 0 stores the number of pairs of row i in slice s of B, MODE 1 reads
// their first position in the pair's list.
template <int MODE>
__global__ __launch_bounds__(KP_THREADS) void kp_pairs_kernel(const KpParams A) {
  __shared__ __attribute__((aligned(16))) float qs[KP_TILE * 2];
  __shared__ __attribute__((aligned(16))) unsigned qmin[KP_TILE];
  const int b = blockIdx.z;
  const long na = pair_rows(A.counts_a, b, A.NA), nb = pair_rows(A.counts_b, b, A.NB);
  const long j_begin = (long)blockIdx.y * A.cnt_per;
  if ((long)blockIdx.x * KP_THREADS >= na || j_begin >= nb) return;  // kp_scan_kernel reads no entry of such a slice
  const long j_end = min(nb, j_begin + A.cnt_per);
  const long i = (long)blockIdx.x * KP_THREADS + threadIdx.x;
  const long o = (long)b * A.NA + i;
  float px = 0.f, py = 0.f;
  unsigned rowmin = KP_NONE;
  bool live = false;
  if (i < na) {
    rowmin = A.min_a[o];
    // (certainty > th) * (D < max_dist) of the reference's mask (matcher.py:756-762)
    live = A.c[o] > A.cert_th && __uint_as_float(rowmin) < A.max_d2;
  }
  long long* entry = A.offs + o * A.cnt_slices + blockIdx.y;
  if (!__syncthreads_or(live)) {  // no row of this block can have a pair
    if (MODE == 0 && i < na) *entry = 0;
    return;
  }
  long base = 0;
  if (live) {
    px = A.p[o * 2 + 0];
    py = A.p[o * 2 + 1];
    if (MODE == 1) base = *entry;
  }
  const float* xb = A.xb + (long)b * A.NB * 2;
  const unsigned* min_b = A.min_b + (long)b * A.NB;
  float sa_x = 1.f, sa_y = 1.f, sb_x = 1.f, sb_y = 1.f;
  if (MODE == 1 && A.sizes) {  // to_pixel_coordinates: W / 2 * (x + 1), H / 2 * (y + 1)
    const float* sz = A.sizes + (long)b * A.sizes_bs;
    sa_y = sz[0] * 0.5f, sa_x = sz[1] * 0.5f, sb_y = sz[2] * 0.5f, sb_x = sz[3] * 0.5f;
  }
  long n = 0;
  for (long j0 = j_begin; j0 < j_end; j0 += KP_TILE) {
    const int cnt = (int)min((long)KP_TILE, j_end - j0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * 2; t += KP_THREADS) qs[t] = xb[j0 * 2 + t];
    // the tile's column minima, filled up to a multiple of 16 with a word that is no live row's minimum
    for (int t = threadIdx.x; t < ((cnt + 15) & ~15); t += KP_THREADS) qmin[t] = t < cnt ? min_b[j0 + t] : KP_NONE;
    __syncthreads();
    if (!live) continue;
    // a row has a handful of pairs at most: 16 column minima per step as four 16-byte LDS reads in flight, compared without a
    // branch, and a closer look only where one of them is the row's minimum
    for (int t16 = 0; t16 < cnt; t16 += 16) {
      uint4 m16[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) m16[g] = *reinterpret_cast<const uint4*>(qmin + t16 + 4 * g);
      bool any = false;
#pragma unroll
      for (int g = 0; g < 4; ++g) any |= (m16[g].x == rowmin) | (m16[g].y == rowmin) | (m16[g].z == rowmin) | (m16[g].w == rowmin);
      if (!any) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint4 m4 = m16[g];
        const int t4 = t16 + 4 * g;
        const unsigned m[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (m[u] != rowmin) continue;
          const int t = t4 + u;
          const float qx = qs[2 * t], qy = qs[2 * t + 1];
          const float dx = px - qx, dy = py - qy;
          if (__float_as_uint(fmaf(dy, dy, dx * dx)) != rowmin) continue;  // the expression of kp_nn_kernel
          if (MODE == 1) {
            const long pos = base + n;
            if (pos < A.M) {
              const long r = ((long)b * A.M + pos) * 2;
              const float ax = A.xa[o * 2 + 0], ay = A.xa[o * 2 + 1];
              A.inds[r + 0] = (int)i;
              A.inds[r + 1] = (int)(j0 + t);
              if (A.sizes) {
                A.kpts_a[r + 0] = sa_x * (ax + 1.0f), A.kpts_a[r + 1] = sa_y * (ay + 1.0f);
                A.kpts_b[r + 0] = sb_x * (qx + 1.0f), A.kpts_b[r + 1] = sb_y * (qy + 1.0f);
              } else {
                A.kpts_a[r + 0] = ax, A.kpts_a[r + 1] = ay;
                A.kpts_b[r + 0] = qx, A.kpts_b[r + 1] = qy;
              }
            }
          }
          ++n;
        }
      }
    }
  }
  if (MODE == 0 && i < na) *entry = n;
}

// ------------------------------------------------------------------ 4. positions, counts and the padding rows; grid (B)
// One workgroup per pair walks the (row, slice) entries in chunks of 1024 consecutive ones (coalesced loads and stores, the next
// chunk's loads issued before this chunk's scan): wg_scan_exclusive per chunk and a running carry.  An entry of a slice that starts
// at or beyond nb was never written and counts as 0.
__global__ __launch_bounds__(1024) void kp_scan_kernel(const KpParams A) {
  __shared__ long long wsum[1024 / WAVE];
  const int b = blockIdx.x;
  const long na = pair_rows(A.counts_a, b, A.NA), nb = pair_rows(A.counts_b, b, A.NB);
  const int S = A.cnt_slices;
  const int live_slices = (int)min((long)S, (nb + A.cnt_per - 1) / A.cnt_per);
  long long* offs = A.offs + (long)b * A.NA * S;
  const long n = na * S;
  auto load = [&](long k) -> long long { return (k < n && (int)((unsigned)k % (unsigned)S) < live_slices) ? offs[k] : 0; };  // n <= 2^23
  long long carry = 0;
  long long v_next = load(threadIdx.x);
  for (long c0 = 0; c0 < n; c0 += 1024) {
    const long k = c0 + threadIdx.x;
    const long long v = v_next;
    v_next = load(k + 1024);  // the next chunk's loads fly during this chunk's scan; its entries are not rewritten yet
    long long tot;
    const long long before = wg_scan_exclusive<1024 / WAVE>(v, wsum, tot);
    if (k < n) offs[k] = carry + before;
    carry += tot;
  }
  const long long total = carry;
  const long cnt = (long)min(total, (long long)A.M);
  if (threadIdx.x == 0) {
    A.total[b] = total;
    A.counts[b] = (int)cnt;
  }
  for (long r = cnt + threadIdx.x; r < A.M; r += 1024) {
    const long q = ((long)b * A.M + r) * 2;
    A.inds[q] = -1, A.inds[q + 1] = -1;
    A.kpts_a[q] = 0.f, A.kpts_a[q + 1] = 0.f;
    A.kpts_b[q] = 0.f, A.kpts_b[q + 1] = 0.f;
  }
}

long blocks_of(long n) { return std::max<long>(1, (n + KP_THREADS - 1) / KP_THREADS); }

// the scanned side's n points in slices of whole tiles, so many that `groups` workgroups per slice fill the device
long slice_points(long n, long groups, long max_slices) {
  const long tiles = std::max<long>(1, (n + KP_TILE - 1) / KP_TILE);
  const long want = std::max<long>(1, std::min<long>(std::min(tiles, max_slices), (KP_TARGET_GROUPS + groups - 1) / groups));
  return std::max<long>(KP_TILE, ((n + want - 1) / want + KP_TILE - 1) / KP_TILE * KP_TILE);
}

long slices_of(long n, long per) { return std::max<long>(1, (n + per - 1) / per); }

bool sizes_ok(int B, long NA, long NB) { return B >= 1 && B <= 65535 && NA >= 0 && NA <= KP_MAX_POINTS && NB >= 0 && NB <= KP_MAX_POINTS; }

// the count slices and the workspace regions of A; returns the bytes of the workspace
size_t carve(Workspace16 ws, int B, long NA, long NB, KpParams& A) {
  const size_t b = (size_t)B, na = (size_t)NA, nb = (size_t)NB;
  A.cnt_per = slice_points(NB, (long)B * blocks_of(NA), KP_COUNT_SLICES);
  A.cnt_slices = (int)slices_of(NB, A.cnt_per);
  A.p = ws.take<float>(b * na * 2);
  A.c = ws.take<float>(b * na);
  A.min_a = ws.take<unsigned>(b * na);
  A.min_b = ws.take<unsigned>(b * nb);
  A.offs = ws.take<long long>(b * na * (size_t)A.cnt_slices);
  return ws.bytes();
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" long roma_op_match_keypoints_workspace(int B, long NA, long NB) {
  if (!sizes_ok(B, NA, NB)) return -1;
  KpParams A;
  return (long)carve(Workspace16(), B, NA, NB, A);
}

extern "C" int roma_op_match_keypoints(const float* x_a, const float* x_b, const int* counts_a, const int* counts_b, const float* warp,
                                       long warp_bs, long warp_rs, const float* certainty, long cert_bs, long cert_rs, const float* sizes,
                                       long sizes_bs, int B, long NA, long NB, int H, int W, float max_dist, float cert_th, long M,
                                       int* inds, float* kpts_a, float* kpts_b, int* counts, long long* total, void* workspace,
                                       long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(B >= 1 && B <= 65535, "match_keypoints: B must lie in [1, 65535]");
  ROMA_REQUIRE(NA >= 0 && NA <= KP_MAX_POINTS && NB >= 0 && NB <= KP_MAX_POINTS, "match_keypoints: NA and NB must lie in [0, 2^20]");
  ROMA_REQUIRE(M >= 1 && M <= 0x7fffffffl, "match_keypoints: M (max_matches) must lie in [1, 2^31 - 1]");
  ROMA_REQUIRE(H > 0 && W > 0 && H <= 32768 && W <= 32768, "match_keypoints: the warp grid (H, W) must lie in [1, 32768]^2");
  ROMA_REQUIRE((x_a || NA == 0) && (x_b || NB == 0) && warp && certainty && inds && kpts_a && kpts_b && counts && total && workspace,
               "match_keypoints: null pointer");
  ROMA_REQUIRE(warp_rs >= 4l * W && warp_rs % 4 == 0 && warp_bs >= (long)(H - 1) * warp_rs + 4l * W && warp_bs % 4 == 0,
               "match_keypoints: warp strides (in floats) must be multiples of 4 with row_stride >= 4 W and batch_stride >= (H - 1) "
               "row_stride + 4 W");
  ROMA_REQUIRE(cert_rs >= W && cert_bs >= (long)(H - 1) * cert_rs + W,
               "match_keypoints: certainty strides (in floats) must have row_stride >= W and batch_stride >= (H - 1) row_stride + W");
  ROMA_REQUIRE(!sizes || sizes_bs == 0 || sizes_bs >= 4, "match_keypoints: sizes stride (in floats) must be 0 (one row for every pair) or >= 4");
  ROMA_REQUIRE(aligned(warp, 16) && aligned(workspace, 16), "match_keypoints: warp and workspace must be 16-byte aligned");
  ROMA_REQUIRE(aligned(x_a, 4) && aligned(x_b, 4) && aligned(counts_a, 4) && aligned(counts_b, 4) && aligned(certainty, 4) &&
                   aligned(sizes, 4) && aligned(inds, 4) && aligned(kpts_a, 4) && aligned(kpts_b, 4) && aligned(counts, 4) &&
                   aligned(total, 8),
               "match_keypoints: a pointer is not aligned to its type");
  ROMA_REQUIRE(max_dist == max_dist && cert_th == cert_th, "match_keypoints: max_dist or cert_th is NaN");
  KpParams A{};
  ROMA_REQUIRE(workspace_bytes >= (long)carve(Workspace16(workspace), B, NA, NB, A),
               "match_keypoints: workspace is too small (roma_op_match_keypoints_workspace)");
  A.xa = x_a, A.xb = x_b, A.counts_a = counts_a, A.counts_b = counts_b;
  A.warp = warp, A.warp_bs = warp_bs, A.warp_rs = warp_rs;
  A.cert = certainty, A.cert_bs = cert_bs, A.cert_rs = cert_rs;
  A.sizes = sizes, A.sizes_bs = sizes_bs;
  A.NA = NA, A.NB = NB, A.M = M, A.H = H, A.W = W;
  A.cert_th = cert_th, A.max_d2 = max_dist * max_dist;
  const long ga = blocks_of(NA), gb = blocks_of(NB);
  A.blocks_a = (int)ga;
  A.nn_per_a = slice_points(NA, (long)B * (ga + gb), 1l << 30);
  A.nn_per_b = slice_points(NB, (long)B * (ga + gb), 1l << 30);
  A.inds = inds, A.kpts_a = kpts_a, A.kpts_b = kpts_b, A.counts = counts, A.total = total;
  const unsigned nn_slices = (unsigned)std::max(slices_of(NA, A.nn_per_a), slices_of(NB, A.nn_per_b));

  hipLaunchKernelGGL(kp_sample_kernel, dim3((unsigned)std::max(ga, gb), B), dim3(KP_THREADS), 0, s, A);
  ROMA_LAUNCH_CHECK();
  {
    ProfScope ps("kp_nn_kernel", 10.0 * (double)B * (double)NA * (double)NB, "flop", s);
    hipLaunchKernelGGL(kp_nn_kernel, dim3((unsigned)(ga + gb), nn_slices, B), dim3(KP_THREADS), 0, s, A);
    ROMA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kp_pairs_kernel<0>, dim3((unsigned)ga, (unsigned)A.cnt_slices, B), dim3(KP_THREADS), 0, s, A);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(kp_scan_kernel, dim3(B), dim3(1024), 0, s, A);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(kp_pairs_kernel<1>, dim3((unsigned)ga, (unsigned)A.cnt_slices, B), dim3(KP_THREADS), 0, s, A);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
