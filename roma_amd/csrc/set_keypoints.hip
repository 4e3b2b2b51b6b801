// Detector-free keypoints from the dense matches of an image set (roma_op_keypoints_from_matches): the endpoints sample_batched
// draws for the P pairs of V <= 8 images are quantised to one keypoint per occupied pixel cell of every view, close keypoints
// of neighbouring cells are merged by a local-maximum test, and the rows are re-indexed to the keypoints that stay - the index
// matches build_tracks reads.  The definition is in include/roma_hip.h; tools/set_keypoints_ref.py restates it in numpy and is
// the oracle of tests/test_gpu_set_keypoints.py.  Everything is integer or max-selection logic on float32 values that every
// stage recomputes from the same inputs by the same expressions (fp contraction off), so the result is a function of the
// inputs alone.
//
// A 64-bit key orders the endpoints: (bits of the certainty) << 32 | (0xFFFFFFFF - ordinal), ordinal = (p N + n) 2 + side.  A
// valid endpoint has a certainty above 0, so 0 is "no candidate"; the ordinal gives back the row and the side, so a cell
// stores its key and nothing else - the position is read again from `matches`.
//
// The workspace holds, per problem, every view's grid padded to a multiple of SKP_BLOCK cells (a workgroup never straddles two
// views): key u64 and idx int32 per cell, one int32 per block of cells, and for one_to_one two u64 per (pair, side, keypoint).
// Seven kernels on the stream, every phase closed by a kernel boundary: what an atomic wrote in L2 is read by the next kernel,
// never by the one that wrote it.
//   clear     key = 0, the one-to-one slots = 0, kpts = NaN, score = 0, info = kept = 0: the workspace need not be zero on entry
//   scatter   one thread per row: both endpoints' keys go to their cells by a 64-bit atomicMax; rows read / invalid are counted
//   suppress  one thread per cell: a candidate survives unless one of the 8 neighbouring cells holds a larger key within the
//             radius; idx = 0 (survives) or -1, and every block of cells writes its number of survivors
//   scan      one workgroup per (problem, view): total = the sum of the view's block counts; above max_kpts a radix select over
//             the survivors' keys (8 passes of 8 bits, the histogram in LDS) finds the K-th largest key, the smaller ones leave
//             and the blocks are counted again; then the exclusive prefix sum of the block counts, in block order
//   number    one thread per cell: a kept survivor's index is its block's prefix plus its rank inside the block (ballots, wave
//             order) - ascending cell id whatever the schedule; kpts and score are written
//   assign    one thread per row: each endpoint takes the nearest kept keypoint of the 3 x 3 cells around it; for one_to_one
//             the row key (bits of the certainty) << 32 | (0xFFFFFFFF - n) goes to the slots of both keypoints by atomicMax
//   finish    one thread per row: a row stays if it holds both of its slots; kept and info are counted
// Integer atomicAdd counts and atomicMax selections do not depend on the order of arrival.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "pair_views.h"
#include "tracks.h"
#include "workgroup.h"
#include "workspace.h"

// nothing here is fused: tools/set_keypoints_ref.py evaluates the same expressions; the one fused multiply-add is written out
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int SET_KPTS_INFO = 6;              // ints per problem in roma_op_keypoints_from_matches' out_info
constexpr int SET_KPTS_MAX_CELL = 64;         // pixels
constexpr int SET_KPTS_MAX_SIZE = 65535;      // H and W of a view
constexpr long SET_KPTS_MAX_GRID = 1l << 22;  // cells of one view
constexpr long SET_KPTS_MAX_CELLS = 1l << 28; // B (G_total + 1024 V): the cells of a call with every view's grid padded to a block
constexpr int SKP_BLOCK = 1024, SKP_WAVES = SKP_BLOCK / WAVE;  // cells per workgroup of the grid kernels, one thread each
constexpr int SKP_ROWS = 256;                                // rows per workgroup of the row kernels
constexpr int SKP_MAX_BLOCKS = (int)(SET_KPTS_MAX_GRID / SKP_BLOCK);  // blocks of one view: the scan keeps them in LDS
typedef unsigned long long u64;

struct SkpParams {
  const float4* matches;
  const float* cert;
  const int* counts;
  int B, V, P, N, K, cell, o2o;
  float r2;      // radius^2 in float32; suppression and the 3 x 3 search are off when radius == 0
  int radius_on;
  float2* kpts;
  float* score;
  int* num_kpts;
  int* total;
  int2* inds;
  int* kept;
  int* info;
  u64* key;   // [B, GP]
  int* idx;   // [B, GP]
  int* bsum;  // [B, NBLK]
  u64* slot;  // [B, P, 2, K]
  long GP;    // padded cells per problem
  int NBLK;   // GP / SKP_BLOCK
  int H[ROMA_TRACKS_MAX_VIEWS], W[ROMA_TRACKS_MAX_VIEWS], Gw[ROMA_TRACKS_MAX_VIEWS], Gh[ROMA_TRACKS_MAX_VIEWS];
  int blk0[ROMA_TRACKS_MAX_VIEWS + 1];  // first block of every view in its problem
  unsigned char pv[ROMA_TRACKS_MAX_PAIRS][2];
};

struct SkpPoint {
  float x, y;
  int cx, cy;
  bool ok;
};

// normalised -> pixels of a W x H view (RegressionMatcher._to_pixel_coordinates' bits) and the cell
__device__ __forceinline__ SkpPoint skp_point(float nx, float ny, int W, int H, int cell) {
  SkpPoint q;
  q.x = ((float)W * 0.5f) * (nx + 1.0f);
  q.y = ((float)H * 0.5f) * (ny + 1.0f);
  q.ok = isfinite(q.x) && isfinite(q.y) && q.x >= 0.0f && q.x < (float)W && q.y >= 0.0f && q.y < (float)H;
  q.cx = q.ok ? (int)floorf(q.x) / cell : 0;
  q.cy = q.ok ? (int)floorf(q.y) / cell : 0;
  return q;
}

__device__ __forceinline__ float skp_d2(float ax, float ay, float bx, float by) {
  const float dx = ax - bx, dy = ay - by;
  return __fmaf_rn(dy, dy, dx * dx);
}

struct SkpRow {
  SkpPoint a, b;
  float c;
  bool read, valid;
};

__device__ __forceinline__ SkpRow skp_row(const SkpParams& S, int b, int p, int n) {
  SkpRow r;
  r.read = false, r.valid = false, r.c = 0.0f;
  r.a.ok = r.b.ok = false;
  const int cnt = S.counts ? min(max(S.counts[(long)b * S.P + p], 0), S.N) : S.N;
  if (n >= cnt) return r;
  r.read = true;
  const long row = ((long)b * S.P + p) * S.N + n;
  const float4 m = S.matches[row];
  r.c = S.cert[row];
  const int va = S.pv[p][0], vb = S.pv[p][1];
  r.a = skp_point(m.x, m.y, S.W[va], S.H[va], S.cell);
  r.b = skp_point(m.z, m.w, S.W[vb], S.H[vb], S.cell);
  r.valid = isfinite(r.c) && r.c > 0.0f && r.a.ok && r.b.ok;
  return r;
}

// the endpoint a key names, in pixels of the W x H view it lies in
__device__ __forceinline__ float2 skp_key_point(const SkpParams& S, int b, u64 key, int W, int H) {
  const unsigned o = 0xFFFFFFFFu - (unsigned)key;
  const float2* m = reinterpret_cast<const float2*>(S.matches + (long)b * S.P * S.N + (o >> 1));
  const float2 e = m[o & 1];
  return make_float2(((float)W * 0.5f) * (e.x + 1.0f), ((float)H * 0.5f) * (e.y + 1.0f));
}

__device__ __forceinline__ int skp_view_of_block(const SkpParams& S, int blk) {
  int v = 0;
#pragma unroll
  for (int u = 1; u < ROMA_TRACKS_MAX_VIEWS; ++u) v += (u < S.V && blk >= S.blk0[u]) ? 1 : 0;
  return v;
}

__global__ __launch_bounds__(256) void skp_clear_kernel(const SkpParams S) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  const long ncell = (long)S.B * S.GP, nslot = S.o2o ? (long)S.B * S.P * 2 * S.K : 0, nk = (long)S.B * S.V * S.K;
  const float nanf_ = __int_as_float(0x7fc00000);
#pragma unroll 1
  for (long i = t; i < ncell; i += step) S.key[i] = 0ull;
#pragma unroll 1
  for (long i = t; i < nslot; i += step) S.slot[i] = 0ull;
#pragma unroll 1
  for (long i = t; i < nk; i += step) {
    S.kpts[i] = make_float2(nanf_, nanf_);
    S.score[i] = 0.0f;
  }
#pragma unroll 1
  for (long i = t; i < (long)S.B * SET_KPTS_INFO; i += step) S.info[i] = 0;
#pragma unroll 1
  for (long i = t; i < (long)S.B * S.P; i += step) S.kept[i] = 0;
}

__global__ __launch_bounds__(SKP_ROWS) void skp_scatter_kernel(const SkpParams S) {
  const int n = blockIdx.x * SKP_ROWS + threadIdx.x, p = blockIdx.y, b = blockIdx.z;
  SkpRow r;
  r.read = r.valid = false;
  if (n < S.N) r = skp_row(S, b, p, n);
  if (r.valid) {
    const unsigned o = ((unsigned)p * (unsigned)S.N + (unsigned)n) * 2u;
    const u64 hi = (u64)__float_as_uint(r.c) << 32;
    const int va = S.pv[p][0], vb = S.pv[p][1];
    u64* grid = S.key + (long)b * S.GP;
    atomicMax(grid + (long)S.blk0[va] * SKP_BLOCK + (r.a.cy * S.Gw[va] + r.a.cx), hi | (u64)(0xFFFFFFFFu - o));
    atomicMax(grid + (long)S.blk0[vb] * SKP_BLOCK + (r.b.cy * S.Gw[vb] + r.b.cx), hi | (u64)(0xFFFFFFFFu - (o + 1u)));
  }
  int* info = S.info + (long)b * SET_KPTS_INFO;
  wave_count_add(info + 0, r.read);
  wave_count_add(info + 1, r.read && !r.valid);
}

__global__ __launch_bounds__(SKP_BLOCK) void skp_suppress_kernel(const SkpParams S) {
  __shared__ int wcnt[SKP_WAVES];
  const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int v = skp_view_of_block(S, blk);
  const int Gw = S.Gw[v], Gh = S.Gh[v], W = S.W[v], H = S.H[v];
  const int g = (blk - S.blk0[v]) * SKP_BLOCK + t;  // the padding beyond Gw Gh holds no key
  const u64* grid = S.key + (long)b * S.GP + (long)S.blk0[v] * SKP_BLOCK;
  const u64 key = grid[g];
  bool surv = key != 0ull, gone = false;
  if (surv && S.radius_on) {
    const float2 q = skp_key_point(S, b, key, W, H);
    const int cy = g / Gw, cx = g - cy * Gw;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
      const int ny = cy + k / 3 - 1, nx = cx + k % 3 - 1;
      if (k == 4 || ny < 0 || ny >= Gh || nx < 0 || nx >= Gw) continue;
      const u64 other = grid[ny * Gw + nx];
      if (other <= key) continue;
      const float2 r = skp_key_point(S, b, other, W, H);
      if (skp_d2(q.x, q.y, r.x, r.y) <= S.r2) gone = true;
    }
    surv = !gone;
  }
  S.idx[(long)b * S.GP + (long)blk * SKP_BLOCK + t] = surv ? 0 : -1;
  wave_count_add(S.info + (long)b * SET_KPTS_INFO + 5, gone);
  const int n = wg_count<SKP_WAVES>(surv, wcnt);
  if (t == 0) S.bsum[(long)b * S.NBLK + blk] = n;
}

__global__ __launch_bounds__(SKP_BLOCK) void skp_scan_kernel(const SkpParams S) {
  constexpr int PER = SKP_MAX_BLOCKS / SKP_BLOCK;  // block counts per thread: 4
  __shared__ int bs[SKP_MAX_BLOCKS];
  __shared__ int hist[256];
  __shared__ int wt[SKP_WAVES];
  const int v = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int nblk = S.blk0[v + 1] - S.blk0[v];  // <= SKP_MAX_BLOCKS
  int* bsum = S.bsum + (long)b * S.NBLK + S.blk0[v];
#pragma unroll
  for (int k = 0; k < PER; ++k) bs[t * PER + k] = t * PER + k < nblk ? bsum[t * PER + k] : 0;
  __syncthreads();
  int mine = 0, total;
#pragma unroll
  for (int k = 0; k < PER; ++k) mine += bs[t * PER + k];
  int before = wg_scan_exclusive<SKP_WAVES>(mine, wt, total);
  if (t == 0) {
    S.total[(long)b * S.V + v] = total;
    S.num_kpts[(long)b * S.V + v] = min(total, S.K);
  }
  if (total > S.K) {  // the same in every thread
    const long base = (long)b * S.GP + (long)S.blk0[v] * SKP_BLOCK;
    const u64* key = S.key + base;
    int* idx = S.idx + base;
    const int cells = nblk * SKP_BLOCK;
    u64 prefix = 0ull;
    int need = S.K;  // the need-th largest key among the survivors that share the prefix
#pragma unroll 1
    for (int pass = 7; pass >= 0; --pass) {
      const int shift = pass * 8;
      __syncthreads();
      if (t < 256) hist[t] = 0;
      __syncthreads();
#pragma unroll 1
      for (int g = t; g < cells; g += SKP_BLOCK) {
        if (idx[g] != 0) continue;
        const u64 k = key[g];
        if (pass == 7 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)(k >> shift) & 255], 1);
      }
      __syncthreads();
      int d = 255, above = 0;
#pragma unroll 1
      for (; d > 0; --d) {
        if (above + hist[d] >= need) break;
        above += hist[d];
      }
      need -= above;
      prefix |= (u64)d << shift;
    }
    // prefix is the K-th largest key: the smaller survivors leave, and the blocks are counted again
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) bs[t * PER + k] = 0;
    __syncthreads();
#pragma unroll 1
    for (int g = t; g < cells; g += SKP_BLOCK) {
      if (idx[g] != 0) continue;
      if (key[g] < prefix) idx[g] = -1;
      else atomicAdd(&bs[g / SKP_BLOCK], 1);
    }
    __syncthreads();
    mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) mine += bs[t * PER + k];
    before = wg_scan_exclusive<SKP_WAVES>(mine, wt, total);
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (t * PER + k < nblk) bsum[t * PER + k] = before;
    before += bs[t * PER + k];
  }
}

__global__ __launch_bounds__(SKP_BLOCK) void skp_number_kernel(const SkpParams S) {
  __shared__ int wcnt[SKP_WAVES];
  const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int v = skp_view_of_block(S, blk);
  const long cell = (long)b * S.GP + (long)blk * SKP_BLOCK + t;
  const bool kept = S.idx[cell] == 0;
  int in_block;  // kept cells of the block: not needed
  const int before = wg_rank<SKP_WAVES>(kept, wcnt, in_block);
  if (!kept) return;
  const int rank = S.bsum[(long)b * S.NBLK + blk] + before;
  S.idx[cell] = rank < S.K ? rank : -1;
  if (rank < S.K) {  // the cut leaves at most K
    const u64 key = S.key[cell];
    const long at = ((long)b * S.V + v) * S.K + rank;
    S.kpts[at] = skp_key_point(S, b, key, S.W[v], S.H[v]);
    S.score[at] = __uint_as_float((unsigned)(key >> 32));
  }
}

// the keypoint of view v an endpoint takes, -1 if none
__device__ __forceinline__ int skp_assign(const SkpParams& S, int b, int v, const SkpPoint& q) {
  const int Gw = S.Gw[v], Gh = S.Gh[v];
  const long base = (long)b * S.GP + (long)S.blk0[v] * SKP_BLOCK;
  const int* idx = S.idx + base;
  if (!S.radius_on) return idx[q.cy * Gw + q.cx];
  const u64* key = S.key + base;
  const float2* kp = S.kpts + ((long)b * S.V + v) * S.K;
  int best = -1;
  float bestd = 0.0f;
  u64 bestkey = 0ull;
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    const int ny = q.cy + k / 3 - 1, nx = q.cx + k % 3 - 1;
    if (ny < 0 || ny >= Gh || nx < 0 || nx >= Gw) continue;
    const int j = idx[ny * Gw + nx];
    if (j < 0) continue;
    const float2 r = kp[j];
    const float d = skp_d2(q.x, q.y, r.x, r.y);
    if (!(d <= S.r2)) continue;
    const u64 kk = key[ny * Gw + nx];
    if (best < 0 || d < bestd || (d == bestd && kk > bestkey)) best = j, bestd = d, bestkey = kk;
  }
  return best;
}

__global__ __launch_bounds__(SKP_ROWS) void skp_assign_kernel(const SkpParams S) {
  const int n = blockIdx.x * SKP_ROWS + threadIdx.x, p = blockIdx.y, b = blockIdx.z;
  SkpRow r;
  r.read = r.valid = false;
  if (n < S.N) r = skp_row(S, b, p, n);
  int ia = -1, ib = -1;
  if (r.valid) {
    ia = skp_assign(S, b, S.pv[p][0], r.a);
    ib = skp_assign(S, b, S.pv[p][1], r.b);
  }
  const bool have = ia >= 0 && ib >= 0;
  wave_count_add(S.info + (long)b * SET_KPTS_INFO + 2, r.valid && !have);
  if (n >= S.N) return;
  const long pair = (long)b * S.P + p;
  S.inds[pair * S.N + n] = have ? make_int2(ia, ib) : make_int2(-1, -1);
  if (have && S.o2o) {
    const u64 rk = ((u64)__float_as_uint(r.c) << 32) | (u64)(0xFFFFFFFFu - (unsigned)n);
    atomicMax(S.slot + (pair * 2 + 0) * S.K + ia, rk);
    atomicMax(S.slot + (pair * 2 + 1) * S.K + ib, rk);
  }
}

__global__ __launch_bounds__(SKP_ROWS) void skp_finish_kernel(const SkpParams S) {
  const int n = blockIdx.x * SKP_ROWS + threadIdx.x, p = blockIdx.y, b = blockIdx.z;
  const long pair = (long)b * S.P + p;
  bool have = false, lost = false;
  if (n < S.N) {
    const int2 r = S.inds[pair * S.N + n];
    have = r.x >= 0;
    if (have && S.o2o) {
      const u64 rk = ((u64)__float_as_uint(S.cert[pair * S.N + n]) << 32) | (u64)(0xFFFFFFFFu - (unsigned)n);
      lost = S.slot[(pair * 2 + 0) * S.K + r.x] != rk || S.slot[(pair * 2 + 1) * S.K + r.y] != rk;
      if (lost) S.inds[pair * S.N + n] = make_int2(-1, -1);
    }
  }
  int* info = S.info + (long)b * SET_KPTS_INFO;
  wave_count_add(info + 3, lost);
  wave_count_add(info + 4, have && !lost);
  wave_count_add(S.kept + pair, have && !lost);
}

// the workspace regions of S for B problems of at most gp padded cells each; returns the bytes of the workspace
size_t skp_carve(Workspace256 ws, int B, long gp, int P, int K, SkpParams& S) {
  S.key = ws.take<u64>((size_t)B * gp);
  S.idx = ws.take<int>((size_t)B * gp);
  S.bsum = ws.take<int>((size_t)B * (gp / SKP_BLOCK));
  S.slot = ws.take<u64>((size_t)B * P * 2 * K);
  return ws.bytes();
}

long skp_padded_bound(int V, long G_total) { return ((G_total + SKP_BLOCK - 1) / SKP_BLOCK + V) * SKP_BLOCK; }

}  // namespace

extern "C" long roma_op_keypoints_from_matches_workspace(int B, int V, int P, int N, long G_total, int K) {
  if (B <= 0 || V <= 0 || V > ROMA_TRACKS_MAX_VIEWS || P < 0 || P > ROMA_TRACKS_MAX_PAIRS || G_total <= 0 || K <= 0 || K > ROMA_TRACKS_MAX_KPTS)
    return 0;
  if (G_total > (long)V * SET_KPTS_MAX_GRID || (long)B * skp_padded_bound(V, G_total) > SET_KPTS_MAX_CELLS) return 0;
  SkpParams S;
  return skp_carve(Workspace256(), B, skp_padded_bound(V, G_total), P, K, S);
}

extern "C" int roma_op_keypoints_from_matches(const float* matches, const float* certainty, const int* counts, const int* pair_views,
                                              const int* sizes, int B, int V, int Pn, int N, int cell, float radius, int K, int one_to_one,
                                              float* out_kpts, float* out_score, int* out_num_kpts, int* out_total, int* out_inds,
                                              int* out_kept, int* out_info, void* ws, long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(out_kpts && out_score && out_num_kpts && out_total && out_info && sizes, "keypoints_from_matches: null pointer");
  ROMA_REQUIRE(V >= 2 && V <= ROMA_TRACKS_MAX_VIEWS, "keypoints_from_matches: need 2 <= V <= 8 views");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "keypoints_from_matches: B must lie in [0, 65535]");
  ROMA_REQUIRE(Pn >= 0 && Pn <= ROMA_TRACKS_MAX_PAIRS, "keypoints_from_matches: need 0 <= P <= 64 pairs");
  ROMA_REQUIRE(N >= 0 && 2l * Pn * N < (1l << 32), "keypoints_from_matches: need N >= 0 and 2 P N below 2^32 rows' endpoints");
  ROMA_REQUIRE((long)B * Pn * N < (1l << 30), "keypoints_from_matches: B * P * N must be below 2^30");
  ROMA_REQUIRE(K >= 1 && K <= ROMA_TRACKS_MAX_KPTS, "keypoints_from_matches: need 1 <= max_kpts <= 65536 keypoints per view");
  ROMA_REQUIRE(cell >= 1 && cell <= SET_KPTS_MAX_CELL, "keypoints_from_matches: cell must lie in [1, 64] pixels");
  ROMA_REQUIRE(radius >= 0.0f && radius <= (float)cell, "keypoints_from_matches: radius must lie in [0, cell] (and not be NaN)");
  ROMA_REQUIRE(one_to_one == 0 || one_to_one == 1, "keypoints_from_matches: one_to_one must be 0 or 1");
  ROMA_REQUIRE(Pn == 0 || (pair_views && out_inds && out_kept && (N == 0 || (matches && certainty))), "keypoints_from_matches: null pointer");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(matches) & 15) == 0, "keypoints_from_matches: matches must be 16-byte aligned");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(out_kpts) & 7) == 0 && (reinterpret_cast<uintptr_t>(out_inds) & 7) == 0,
               "keypoints_from_matches: kpts and inds must be 8-byte aligned");
  SkpParams S = {};
  long gtot = 0;
  int blocks = 0;
  for (int v = 0; v < V; ++v) {
    const int H = sizes[2 * v], W = sizes[2 * v + 1];
    ROMA_REQUIRE(H >= 1 && H <= SET_KPTS_MAX_SIZE && W >= 1 && W <= SET_KPTS_MAX_SIZE, "keypoints_from_matches: image sizes must lie in [1, 65535]");
    const int gw = (W + cell - 1) / cell, gh = (H + cell - 1) / cell;
    ROMA_REQUIRE((long)gw * gh <= SET_KPTS_MAX_GRID, "keypoints_from_matches: a view has more than 2^22 cells; use a larger cell");
    S.H[v] = H, S.W[v] = W, S.Gw[v] = gw, S.Gh[v] = gh;
    S.blk0[v] = blocks;
    blocks += (gw * gh + SKP_BLOCK - 1) / SKP_BLOCK;
    gtot += (long)gw * gh;
  }
  for (int v = V; v <= ROMA_TRACKS_MAX_VIEWS; ++v) S.blk0[v] = blocks;
  ROMA_REQUIRE((long)B * skp_padded_bound(V, gtot) <= SET_KPTS_MAX_CELLS,
               "keypoints_from_matches: B * (cells of all views + 1024 V) must not exceed 2^28; use a larger cell or fewer problems");
  if (int rc = check_pairs("keypoints_from_matches", pair_views, V, Pn, S.pv)) return rc;  // whether or not a row will be read
  if (B == 0) return 0;
  ROMA_REQUIRE(ws && ws_bytes >= (size_t)roma_op_keypoints_from_matches_workspace(B, V, Pn, N, gtot, K), "keypoints_from_matches: workspace too small");
  // laid out for the cells there are: never more than the bound the workspace entry sizes for
  S.GP = (long)blocks * SKP_BLOCK;
  S.NBLK = blocks;
  skp_carve(Workspace256(ws), B, S.GP, Pn, K, S);
  S.matches = reinterpret_cast<const float4*>(matches);
  S.cert = certainty;
  S.counts = counts;
  S.B = B, S.V = V, S.P = Pn, S.N = N, S.K = K, S.cell = cell, S.o2o = one_to_one;
  S.r2 = radius * radius;
  S.radius_on = radius > 0.0f ? 1 : 0;
  S.kpts = reinterpret_cast<float2*>(out_kpts);
  S.score = out_score;
  S.num_kpts = out_num_kpts, S.total = out_total;
  S.inds = reinterpret_cast<int2*>(out_inds);
  S.kept = out_kept, S.info = out_info;
  const bool rows = Pn > 0 && N > 0;
  const dim3 row_grid((N + SKP_ROWS - 1) / SKP_ROWS, Pn > 0 ? Pn : 1, B), cell_grid(blocks, B);
  const double work = (double)B * ((double)Pn * N + (double)S.GP);
  {
    const long words = std::max((long)B * S.GP, (long)B * Pn * 2 * K);
    ProfScope ps("skp_clear_kernel", work, "B", s);
    hipLaunchKernelGGL(skp_clear_kernel, dim3((unsigned)std::min<long>((words + 255) / 256, 4096)), dim3(256), 0, s, S);
    ROMA_LAUNCH_CHECK();
  }
  if (rows) {
    ProfScope ps("skp_scatter_kernel", work, "B", s);
    hipLaunchKernelGGL(skp_scatter_kernel, row_grid, dim3(SKP_ROWS), 0, s, S);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("skp_suppress_kernel", work, "B", s);
    hipLaunchKernelGGL(skp_suppress_kernel, cell_grid, dim3(SKP_BLOCK), 0, s, S);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("skp_scan_kernel", work, "B", s);
    hipLaunchKernelGGL(skp_scan_kernel, dim3(V, B), dim3(SKP_BLOCK), 0, s, S);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("skp_number_kernel", work, "B", s);
    hipLaunchKernelGGL(skp_number_kernel, cell_grid, dim3(SKP_BLOCK), 0, s, S);
    ROMA_LAUNCH_CHECK();
  }
  if (rows) {
    {
      ProfScope ps("skp_assign_kernel", work, "B", s);
      hipLaunchKernelGGL(skp_assign_kernel, row_grid, dim3(SKP_ROWS), 0, s, S);
      ROMA_LAUNCH_CHECK();
    }
    ProfScope ps("skp_finish_kernel", work, "B", s);
    hipLaunchKernelGGL(skp_finish_kernel, row_grid, dim3(SKP_ROWS), 0, s, S);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace roma
