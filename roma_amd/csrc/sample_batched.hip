// RegressionMatcher.sample (romatch/models/matcher.py:598-629) applied to each pair of a batch separately, in one enqueue of a
// fixed number of launches with no host read: the thresholded certainty, both draws without replacement, both gathers and the
// density between them.  The pair is a grid axis of every kernel; pair b draws from seeds[b].
//
// The draws are the exponential race of sampling.hip (same mix64 use, same u, key = min(-log(u) / w, 3e38), +inf for w <= 0) and
// its 3-pass radix select, with one SelState-like record and one 2048-bin histogram per pair.  Unlike the single-pair path the
// result is a function of (inputs, seeds[b]) alone - the same on every run, for every B and wherever the pair sits in the batch:
//   * which of the entries that hold the k-th key are taken does not depend on arrival order.  The keys are counted in chunks of
//     TIE_CHUNK indices, one workgroup per pair walks the chunk counts and then the one chunk that holds the cut in index order
//     with a block prefix count, and the compaction takes key < T || (key == T && index <= cut): lowest indices first, the +inf
//     filler entries of a pair with fewer than k positive weights included;
//   * the compaction's own order (an atomic cursor) is arbitrary, but the all-pairs rank by (key, index) that follows puts the
//     sample in draw order whatever it was;
//   * the density adds no float atomically: the reference rows are cut into slices whose number depends on k alone, every
//     (query, slice) partial sum goes to the workspace and an epilogue adds them in slice order.  Integer atomics (histograms,
//     the count of positive weights, the cursor) give the same totals in any order.
// The density is kde_kernel<true>'s loop (kde.hip): coordinates rounded to fp16, f32 accumulation, v_exp_f32 with
// coef = -log2(e) / (2 * 0.1^2), 1024 reference rows per LDS tile read as wave-wide broadcasts.
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "sampling.h"
#include "workgroup.h"
#include "workspace.h"

namespace roma {
namespace {

// the second draw of pair b runs on seeds[b] ^ SAMPLE_SECOND_DRAW_SEED (the multiplier of Knuth's MMIX generator)
constexpr unsigned long long SAMPLE_SECOND_DRAW_SEED = 0x5851f42d4c957f2dull;
// largest first-draw size: the all-pairs order of sampling.hip (ORDER_ALLPAIRS_MAX); its bitonic path is not batched
constexpr long SAMPLE_BATCHED_MAX_K = 65536;

struct PairState {      // one per pair and draw, at the head of the workspace
  unsigned prefix;      // bits of the k-th key fixed so far; after the third pass the key T itself
  unsigned remaining;   // rank of the k-th key inside the current prefix bucket (1-based)
  unsigned out_count;   // compaction cursor
  unsigned ties_left;   // how many entries with key == T belong to the sample
  unsigned n_positive;  // number of weights > 0 (first draw)
  unsigned cut;         // entries with key == T are taken up to this index
  unsigned pad[2];
};

constexpr int TIE_CHUNK = 2048;   // indices per workgroup of the tie count
constexpr int KDE_TILE = 1024;    // reference rows per LDS tile
constexpr int KDE_MAX_SLICES = 8;
constexpr int TIE_WAVES = 256 / WAVE;  // of the workgroup that finds the cut

__device__ __forceinline__ float round_to_half(float v) { return (float)(_Float16)v; }

// race_keys_kernel's key (sampling.hip), term for term
__device__ __forceinline__ float race_key(float w, uint64_t seed, long i) {
  float key = __int_as_float(0x7f800000);  // +inf
  if (w > 0.f) {
    const uint64_t r = mix64(mix64(seed + 0x9e3779b97f4a7c15ull * (uint64_t)(i + 1)) ^ seed);
    const float u = ((float)(r >> 41) + 0.5f) * (1.0f / 8388608.0f);
    key = -__logf(u) / w;
    key = fminf(key, 3.0e38f);
  }
  return key;
}

// (key bits, index): ordered like (key, index) for the non-negative keys of the race
__device__ __forceinline__ unsigned long long pack_key(float key, int idx) {
  return ((unsigned long long)__float_as_uint(key) << 32) | (unsigned long long)(unsigned)idx;
}

// grid (8, B): clears the pair's histogram and sets the states of both draws
__global__ __launch_bounds__(256) void sample_init_kernel(PairState* st1, PairState* st2, unsigned* hist, unsigned k, unsigned m) {
  const int b = blockIdx.y;
  hist[(long)b * 2048 + blockIdx.x * 256 + threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const PairState a = {0, k, 0, 0, 0, 0, {0, 0}}, c = {0, m, 0, 0, 0, 0, {0, 0}};
    st1[b] = a;
    st2[b] = c;
  }
}

// first draw's keys from the (thresholded) certainty; grid (n / 256, B)
__global__ __launch_bounds__(256) void sample_keys_kernel(const float* __restrict__ cert, const unsigned long long* __restrict__ seeds,
                                                          long n, int threshold, float thresh, float* __restrict__ keys, PairState* st) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool positive = false;
  if (i < n) {
    float w = cert[(long)b * n + i];
    if (threshold && w > thresh) w = 1.f;
    positive = w > 0.f;
    keys[(long)b * n + i] = race_key(w, seeds[b], i);
  }
  const unsigned long long mask = __ballot(positive);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&st[b].n_positive, (unsigned)__popcll(mask));
}

// race_hist_kernel per pair; grid (blocks, B)
__global__ __launch_bounds__(256) void sample_hist_kernel(const float* __restrict__ keys, long n, int shift, int bits, int pass,
                                                          const PairState* st, unsigned* __restrict__ hist) {
  __shared__ unsigned lh[2048];
  const int b = blockIdx.y;
  const float* kb = keys + (long)b * n;
  const int nb = 1 << bits;
  for (int i = threadIdx.x; i < nb; i += 256) lh[i] = 0;
  __syncthreads();
  const unsigned prefix = st[b].prefix;
  const int hi_shift = shift + bits;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const unsigned key = __float_as_uint(kb[i]);
    if (pass == 0 || (key >> hi_shift) == (prefix >> hi_shift)) atomicAdd(&lh[(key >> shift) & (nb - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 256)
    if (lh[i]) atomicAdd(&hist[(long)b * 2048 + i], lh[i]);
}

// race_scan_kernel per pair; grid (1, B)
__global__ __launch_bounds__(256) void sample_scan_kernel(unsigned* __restrict__ hist, int shift, int bits, int last, PairState* st) {
  __shared__ unsigned part[256];
  const int b = blockIdx.y;
  unsigned* hb = hist + (long)b * 2048;
  const int nb = 1 << bits, per = nb / 256;
  unsigned s = 0;
  for (int j = 0; j < per; ++j) s += hb[threadIdx.x * per + j];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned rem = st[b].remaining, acc = 0;
    int t = 0;
    while (t < 255 && acc + part[t] < rem) acc += part[t++];
    int bk = t * per;
    while (bk < (t + 1) * per - 1 && acc + hb[bk] < rem) acc += hb[bk++];
    st[b].prefix |= (unsigned)bk << shift;
    st[b].remaining = rem - acc;
    if (last) st[b].ties_left = rem - acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 256) hb[i] = 0;
}

// number of keys equal to T in each chunk of TIE_CHUNK indices; grid (chunks, B)
__global__ __launch_bounds__(256) void sample_tie_count_kernel(const float* __restrict__ keys, long n, const PairState* st,
                                                               unsigned* __restrict__ cnt) {
  __shared__ unsigned wsum[4];
  const int b = blockIdx.y;
  const float* kb = keys + (long)b * n;
  const unsigned T = st[b].prefix;
  const long base = (long)blockIdx.x * TIE_CHUNK;
  unsigned c = 0;
  for (int r = 0; r < TIE_CHUNK / 256; ++r) {
    const long i = base + r * 256 + threadIdx.x;
    if (i < n && __float_as_uint(kb[i]) == T) ++c;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_down(c, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[(long)b * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup per pair: the index `cut` with exactly ties_left keys equal to T at indices <= cut; grid (1, B)
__global__ __launch_bounds__(256) void sample_tie_cut_kernel(const float* __restrict__ keys, long n, PairState* st,
                                                             const unsigned* __restrict__ cnt, int nchunks) {
  __shared__ unsigned wtot[TIE_WAVES];
  __shared__ unsigned found[2];  // the chunk that holds the cut, and how many of its ties are taken
  const int b = blockIdx.y;
  const float* kb = keys + (long)b * n;
  const unsigned* cb = cnt + (long)b * nchunks;
  const unsigned T = st[b].prefix, need_all = st[b].ties_left;
  if (threadIdx.x == 0) found[0] = 0xffffffffu, found[1] = 0;
  __syncthreads();
  unsigned running = 0;
  for (int c0 = 0; c0 < nchunks; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    const unsigned v = c < nchunks ? cb[c] : 0u;
    unsigned total;
    const unsigned excl = running + wg_scan_exclusive<TIE_WAVES>(v, wtot, total);
    if (running + total >= need_all) {  // the same for every thread
      if (excl < need_all && need_all <= excl + v) found[0] = (unsigned)c, found[1] = need_all - excl;
      break;
    }
    running += total;
  }
  __syncthreads();
  const unsigned chunk = found[0], need = found[1];
  if (chunk == 0xffffffffu) {  // fewer ties than the histogram counted: cannot happen; every tie is taken then
    if (threadIdx.x == 0) st[b].cut = (unsigned)(n - 1);
    return;
  }
  const long base = (long)chunk * TIE_CHUNK;
  unsigned run = 0;
  for (int r = 0; r < TIE_CHUNK / 256; ++r) {
    const long i = base + r * 256 + threadIdx.x;
    const unsigned f = (i < n && __float_as_uint(kb[i]) == T) ? 1u : 0u;
    unsigned total;
    const unsigned incl = run + wg_scan_exclusive<TIE_WAVES>(f, wtot, total) + f;
    if (f && incl == need) st[b].cut = (unsigned)i;
    run += total;
  }
}

// indices of the k smallest keys, ties by index, in arbitrary order; grid (n / 256, B)
__global__ __launch_bounds__(256) void sample_compact_kernel(const float* __restrict__ keys, long n, PairState* st, int* __restrict__ sel,
                                                             long k) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned key = __float_as_uint(keys[(long)b * n + i]), T = st[b].prefix;
  if (key < T || (key == T && (unsigned)i <= st[b].cut)) {
    const unsigned pos = atomicAdd(&st[b].out_count, 1u);
    if ((long)pos < k) sel[(long)b * k + pos] = (int)i;
  }
}

// race_order_kernel per pair with the gather in it: rank r of every selected row among the pair's (key, index) words, then
// dst row r = source row.  src_map: the source rows' indices into the pair's n input rows (second draw), or null (first draw:
// the source row is the input row).  grid (k / 256, B)
__global__ __launch_bounds__(256) void sample_order_gather_kernel(
    const float* __restrict__ keys, long n, const int* __restrict__ sel, long k, const float* __restrict__ src_m,
    const float* __restrict__ src_c, const int* __restrict__ src_map, int threshold, float thresh, float* __restrict__ dst_m,
    float* __restrict__ dst_c, int* __restrict__ dst_idx32, long long* __restrict__ dst_idx_a, long long* __restrict__ dst_idx_b,
    const PairState* st_first, int* __restrict__ counts, int m) {
  __shared__ unsigned long long tile[256];
  const int b = blockIdx.y;
  const float* kb = keys + (long)b * n;
  const int* sb = sel + (long)b * k;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  int mi = 0;
  if (i < k) {
    mi = sb[i];
    if ((unsigned)mi >= (unsigned long)n) mi = 0;  // never out of the pair's rows, whatever the workspace held
  }
  const unsigned long long mine = i < k ? pack_key(kb[mi], mi) : 0ull;
  unsigned rank = 0;
  for (long j0 = 0; j0 < k; j0 += 256) {
    const long j = j0 + threadIdx.x;
    unsigned long long v = ~0ull;  // beyond k: behind every entry
    if (j < k) {
      int mj = sb[j];
      if ((unsigned)mj >= (unsigned long)n) mj = 0;
      v = pack_key(kb[mj], mj);
    }
    __syncthreads();
    tile[threadIdx.x] = v;
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < 256; ++t) rank += tile[t] < mine ? 1u : 0u;
  }
  if (counts && blockIdx.x == 0 && threadIdx.x == 0) counts[b] = (int)min((unsigned)m, st_first[b].n_positive);
  if (i >= k || (long)rank >= k) return;
  const long src = (long)b * n + mi, dst = (long)b * k + rank;
  float c = src_c[src];
  if (threshold && c > thresh) c = 1.f;
  *reinterpret_cast<f32x4*>(dst_m + dst * 4) = *reinterpret_cast<const f32x4*>(src_m + src * 4);
  dst_c[dst] = c;
  const int orig = src_map ? src_map[src] : mi;
  if (dst_idx32) dst_idx32[dst] = orig;
  if (dst_idx_a) dst_idx_a[dst] = orig;
  if (dst_idx_b) dst_idx_b[dst] = orig;
}

// kde_kernel<true>'s loop over the pair's k stage rows; the partial sum of (query i, slice) goes to partial[b][slice][i].
// grid (k / 256, slices, B)
__global__ __launch_bounds__(256) void sample_kde_kernel(const float* __restrict__ stage_m, long k, float coef, float* __restrict__ partial,
                                                         long ref_per_slice) {
  __shared__ __attribute__((aligned(16))) f32x4 ys[KDE_TILE];
  const int b = blockIdx.z;
  const float* x = stage_m + (long)b * k * 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  f32x4 xi = {0.f, 0.f, 0.f, 0.f};
  if (i < k) xi = *reinterpret_cast<const f32x4*>(x + i * 4);
#pragma unroll
  for (int c = 0; c < 4; ++c) xi[c] = round_to_half(xi[c]);
  const long j_begin = (long)blockIdx.y * ref_per_slice;
  const long j_end = min(k, j_begin + ref_per_slice);
  float acc = 0.f;
  for (long j0 = j_begin; j0 < j_end; j0 += KDE_TILE) {
    const int cnt = (int)min((long)KDE_TILE, j_end - j0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += 256) {
      f32x4 y = *reinterpret_cast<const f32x4*>(x + (j0 + t) * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = round_to_half(y[c]);
      ys[t] = y;
    }
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < cnt; ++t) {
      const f32x4 y = ys[t];
      const float d0 = xi[0] - y[0], d1 = xi[1] - y[1], d2 = xi[2] - y[2], d3 = xi[3] - y[3];
      const float q = fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, d0 * d0)));
      acc += __builtin_amdgcn_exp2f(q * coef);
    }
  }
  if (i < k) partial[((long)b * gridDim.y + blockIdx.y) * k + i] = acc;
}

// density = the slices' partial sums in slice order; second draw's key from p = 1 / (density + 1), 1e-7 where density < 10,
// 0 for a filler row (certainty not positive).  grid (k / 256, B)
__global__ __launch_bounds__(256) void sample_density_keys_kernel(const float* __restrict__ partial, int slices, long k,
                                                                  const float* __restrict__ stage_c,
                                                                  const unsigned long long* __restrict__ seeds, float* __restrict__ keys2,
                                                                  float* __restrict__ out_density) {
  const int b = blockIdx.y;
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= k) return;
  float d = 0.f;
  for (int s = 0; s < slices; ++s) d += partial[((long)b * slices + s) * k + j];
  if (out_density) out_density[(long)b * k + j] = d;
  float p = 1.0f / (d + 1.0f);
  if (d < 10.f) p = 1e-7f;
  if (!(stage_c[(long)b * k + j] > 0.f)) p = 0.f;
  keys2[(long)b * k + j] = race_key(p, seeds[b] ^ SAMPLE_SECOND_DRAW_SEED, j);
}

struct Sizes {
  long k, m, chunks, slices, per;
};

bool sizes(long n, long num, int balanced, Sizes* z) {
  z->m = std::min(num, n);
  z->k = !balanced ? z->m : z->m > n / 4 ? n : 4 * z->m;  // min(4 num, n) without overflow
  z->chunks = (n + TIE_CHUNK - 1) / TIE_CHUNK;
  // reference slices of the density: a function of k alone
  const long tiles = (z->k + KDE_TILE - 1) / KDE_TILE;
  const long want = std::max<long>(1, std::min<long>(tiles, KDE_MAX_SLICES));
  z->per = ((z->k + want - 1) / want + KDE_TILE - 1) / KDE_TILE * KDE_TILE;
  z->slices = (z->k + z->per - 1) / z->per;
  return z->k <= SAMPLE_BATCHED_MAX_K;
}

struct Carve {  // the workspace; stage_*, partial and keys2 only in the balanced modes (NULL otherwise)
  PairState *st1, *st2;
  unsigned *hist, *cnt;
  float *keys1, *stage_m, *stage_c, *partial, *keys2;
  int *sel, *stage_idx;
  size_t bytes;
};

Carve carve(Workspace16 ws, int B, long n, const Sizes& z, int balanced) {
  Carve c{};
  const size_t b = (size_t)B, k = (size_t)z.k;
  c.st1 = ws.take<PairState>(b);
  c.st2 = ws.take<PairState>(b);
  c.hist = ws.take<unsigned>(b * 2048);
  c.cnt = ws.take<unsigned>(b * (size_t)z.chunks);
  c.keys1 = ws.take<float>(b * (size_t)n);
  c.sel = ws.take<int>(b * k);
  if (balanced) {
    c.stage_idx = ws.take<int>(b * k);
    c.stage_m = ws.take<float>(b * k * 4);
    c.stage_c = ws.take<float>(b * k);
    c.partial = ws.take<float>(b * (size_t)z.slices * k);
    c.keys2 = ws.take<float>(b * k);
  }
  c.bytes = ws.bytes();
  return c;
}

// the k smallest of each pair's n keys into sel [B, k] (hist zero on entry and on exit; st holds remaining = k)
int select_launch(const float* keys, long n, long k, PairState* st, unsigned* hist, unsigned* cnt, int* sel, int B, hipStream_t s) {
  const unsigned gn = (unsigned)((n + 255) / 256), gh = (unsigned)std::min<long>((n + 255) / 256, 1024);
  const int chunks = (int)((n + TIE_CHUNK - 1) / TIE_CHUNK);
  const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
  for (int p = 0; p < 3; ++p) {
    hipLaunchKernelGGL(sample_hist_kernel, dim3(gh, B), dim3(256), 0, s, keys, n, shifts[p], bits[p], p, st, hist);
    ROMA_LAUNCH_CHECK();
    hipLaunchKernelGGL(sample_scan_kernel, dim3(1, B), dim3(256), 0, s, hist, shifts[p], bits[p], p == 2 ? 1 : 0, st);
    ROMA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sample_tie_count_kernel, dim3(chunks, B), dim3(256), 0, s, keys, n, st, cnt);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(sample_tie_cut_kernel, dim3(1, B), dim3(256), 0, s, keys, n, st, cnt, chunks);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(sample_compact_kernel, dim3(gn, B), dim3(256), 0, s, keys, n, st, sel, k);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" long roma_op_sample_matches_workspace(int B, long n, long num, int balanced) {
  if (B <= 0 || n <= 0 || num <= 0) return 0;
  Sizes z;
  sizes(n, num, balanced, &z);
  return carve(Workspace16(), B, n, z, balanced).bytes;
}

extern "C" int roma_op_sample_matches(const float* matches, const float* certainty, const unsigned long long* seeds, int B, long n,
                                      long num, int threshold, float thresh, int balanced, float* out_matches, float* out_certainty,
                                      int* out_counts, long long* out_idx, long long* out_first_idx, float* out_density, void* ws,
                                      long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(matches && certainty && seeds && out_matches && out_certainty, "sample_matches: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "sample_matches: B must lie in [0, 65535]");
  ROMA_REQUIRE(n >= 0 && num >= 0, "sample_matches: n and num must not be negative");
  if (B == 0 || n == 0 || num == 0) return 0;
  ROMA_REQUIRE(n < (1l << 31), "sample_matches: n too large (n must be below 2^31)");
  Sizes z;
  ROMA_REQUIRE(sizes(n, num, balanced, &z),
               "sample_matches: the first draw takes k = min(4 num, n) rows in the balanced modes (min(num, n) otherwise) and k > 65536 "
               "is not batched (num <= 16384 in the balanced modes); use sample() per pair");
  ROMA_REQUIRE(ws, "sample_matches: null pointer (workspace)");
  const Carve c = carve(Workspace16(ws), B, n, z, balanced);
  ROMA_REQUIRE(ws_bytes >= c.bytes, "sample_matches: workspace too small (roma_op_sample_matches_workspace)");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(matches) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_matches) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
               "sample_matches: matches, out_matches and workspace must be 16-byte aligned");
  const long k = z.k, m = z.m;
  const unsigned gk = (unsigned)((k + 255) / 256);

  hipLaunchKernelGGL(sample_init_kernel, dim3(8, B), dim3(256), 0, s, c.st1, c.st2, c.hist, (unsigned)k, (unsigned)m);
  ROMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(sample_keys_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, certainty, seeds, n, threshold, thresh,
                     c.keys1, c.st1);
  ROMA_LAUNCH_CHECK();
  if (int e = select_launch(c.keys1, n, k, c.st1, c.hist, c.cnt, c.sel, B, s)) return e;
  if (!balanced) {  // the first draw is the sample (k = m): the filler already sorts last
    hipLaunchKernelGGL(sample_order_gather_kernel, dim3(gk, B), dim3(256), 0, s, c.keys1, n, c.sel, k, matches, certainty,
                       (const int*)nullptr, threshold, thresh, out_matches, out_certainty, (int*)nullptr, out_idx, out_first_idx, c.st1,
                       out_counts, (int)m);
    ROMA_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(sample_order_gather_kernel, dim3(gk, B), dim3(256), 0, s, c.keys1, n, c.sel, k, matches, certainty, (const int*)nullptr,
                     threshold, thresh, c.stage_m, c.stage_c, c.stage_idx, out_first_idx, (long long*)nullptr, c.st1, (int*)nullptr, (int)m);
  ROMA_LAUNCH_CHECK();
  {
    const float std_ = 0.1f, coef = -1.4426950408889634f / (2.0f * std_ * std_);
    ProfScope ps("sample_kde_kernel", 10.0 * (double)B * (double)k * (double)k, "flop", s);
    hipLaunchKernelGGL(sample_kde_kernel, dim3(gk, (unsigned)z.slices, B), dim3(256), 0, s, c.stage_m, k, coef, c.partial, z.per);
    ROMA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sample_density_keys_kernel, dim3(gk, B), dim3(256), 0, s, c.partial, (int)z.slices, k, c.stage_c, seeds, c.keys2,
                     out_density);
  ROMA_LAUNCH_CHECK();
  if (int e = select_launch(c.keys2, k, m, c.st2, c.hist, c.cnt, c.sel, B, s)) return e;
  hipLaunchKernelGGL(sample_order_gather_kernel, dim3((unsigned)((m + 255) / 256), B), dim3(256), 0, s, c.keys2, k, c.sel, m, c.stage_m, c.stage_c,
                     c.stage_idx, 0, 0.f, out_matches, out_certainty, (int*)nullptr, out_idx, (long long*)nullptr, c.st1, out_counts, (int)m);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
