// Multi-view tracks from pairwise index matches (roma_op_build_tracks): what joins match_keypoints over the pairs of V <= 8 images
// into the [V, N] observation table bundle_adjust and triangulate_views read.  tools/tracks_ref.py restates the definition with
// a numpy union-find and is the oracle of tests/test_gpu_views.py.
//
// Nodes are the keypoints, id = v K + i; edges are the rows of inds whose two indices are inside [0, num_kpts).  A connected
// component is a track when it has at least min_views nodes and no view twice; a component with two keypoints of one view is
// dropped whole (OpenMVG's rule).  Tracks are numbered in ascending order of their smallest node id, so the result depends on
// the edge SET alone.
//
// One workgroup of 1024 threads per problem runs everything in one launch; it never waits on another workgroup.  Four int32 per
// node live in the workspace (label, slot, view mask, conflict).  Phases, each closed by a workgroup barrier:
//   labels    label[u] = u.  A round hooks, for every edge whose ends have different labels, the larger label under the
//             smaller (atomicMin on label[larger]: the only atomic of the kernel), then jumps pointers (label[u] = label[label[u]])
//             until every node points at a root.  A label only ever points at a smaller id of the same component, so the
//             forest has no cycle; a round that hooks anything removes at least one root, so there are fewer than V K rounds,
//             and the loop ends at the first round that hooks nothing.  Then every label is the smallest id of its component
//             whatever the schedule was.  Jumping halves the depth: at most 20 passes for 2^19 nodes.
//   views     view by view: every keypoint of the view writes its id into slot[label]; after the barrier the one that finds its
//             own id there sets the view's bit in mask[label], the others set conflict[label].  No atomics: the winner of the
//             race is arbitrary, the bits are not.
//   numbers   every wave walks one contiguous segment of the ids, 64 at a time; the roots that are tracks are counted by ballot,
//             the waves' totals are added in wave order, a second walk writes the track number into slot[root].
//   fill      tracks = -1 and kpts = NaN everywhere, then every keypoint of a track below max_tracks writes its own cell.
#include <math.h>
#include <stdint.h>

#include "../../include/roma_hip.h"
#include "common.h"
#include "pair_views.h"
#include "tracks.h"
#include "workgroup.h"
#include "workspace.h"

namespace roma {
namespace {

constexpr int BUILD_TRACKS_INFO = 4;  // ints per problem in roma_op_build_tracks' out_info
constexpr int TRK_THREADS = 1024, TRK_WAVES = TRK_THREADS / WAVE;
constexpr int TRK_ARRAYS = 4;  // label, slot, mask, conflict

struct TrkPairs {
  unsigned char v[ROMA_TRACKS_MAX_PAIRS][2];
};

struct TrkParams {
  const int2* inds;
  const int* match_counts;
  const int* num_kpts;
  const float2* x;
  int V, K, P, M, T, min_views;
  int* tracks;
  float2* kpts;
  int* counts;
  int* total;
  int* info;
  int* ws;
  long per_problem, per_array;  // ints
  TrkPairs pv;
};

long trk_array_ints(int V, int K) { return (long)(align256(sizeof(int) * (size_t)V * K) / sizeof(int)); }

// the workspace of P: TRK_ARRAYS padded arrays per problem; returns the bytes of the workspace
size_t trk_carve(Workspace256 ws, int B, int V, int K, TrkParams& P) {
  P.per_array = trk_array_ints(V, K);
  P.per_problem = TRK_ARRAYS * P.per_array;
  P.ws = ws.take<int>((size_t)B * P.per_problem);
  return ws.bytes();
}

// A label as memory holds it.  Labels are lowered by atomics, which execute in L2; every read of one goes there too (a relaxed
// agent-scope load bypasses the CU's L1), so no phase depends on what the L1 does with a line an atomic has rewritten.
__device__ __forceinline__ int trk_label(const int* lab, int u) { return __hip_atomic_load(lab + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(TRK_THREADS) void build_tracks_kernel(const TrkParams P) {
  __shared__ int nk[ROMA_TRACKS_MAX_VIEWS];
  __shared__ int sh[TRK_WAVES];
  __shared__ int wtot[3][TRK_WAVES];
  const int b = blockIdx.x, t = threadIdx.x;
  const int V = P.V, K = P.K, M = P.M, n = V * K;  // n <= 2^19
  int* lab = P.ws + (long)b * P.per_problem;
  int* slot = lab + P.per_array;
  int* mask = slot + P.per_array;
  int* conf = mask + P.per_array;
  const int2* rows = P.inds + (long)b * P.P * M;
  if (t < V) nk[t] = P.num_kpts ? min(max(P.num_kpts[(long)b * V + t], 0), K) : K;
#pragma unroll 1
  for (int u = t; u < n; u += TRK_THREADS) {
    lab[u] = u;
    slot[u] = -1;
    mask[u] = 0;
    conf[u] = 0;
  }
  __syncthreads();

  // rows used and ignored
  int used = 0, ignored = 0;
#pragma unroll 1
  for (int p = 0; p < P.P; ++p) {
    const int mc = P.match_counts ? min(max(P.match_counts[(long)b * P.P + p], 0), M) : M;
    const unsigned ka = (unsigned)nk[P.pv.v[p][0]], kb = (unsigned)nk[P.pv.v[p][1]];
#pragma unroll 1
    for (int m = t; m < mc; m += TRK_THREADS) {
      const int2 r = rows[(long)p * M + m];
      const bool ok = (unsigned)r.x < ka && (unsigned)r.y < kb;  // a negative index is a huge unsigned one
      used += ok ? 1 : 0;
      ignored += ok ? 0 : 1;
    }
  }
  used = wg_sum<TRK_WAVES>(used, sh);
  ignored = wg_sum<TRK_WAVES>(ignored, sh);

  // labels: min-label hooking and pointer jumping
#pragma unroll 1
  for (int round = 0; round < n; ++round) {
    int hooked = 0;
#pragma unroll 1
    for (int p = 0; p < P.P; ++p) {
      const int mc = P.match_counts ? min(max(P.match_counts[(long)b * P.P + p], 0), M) : M;
      const int va = P.pv.v[p][0], vb = P.pv.v[p][1];
      const unsigned ka = (unsigned)nk[va], kb = (unsigned)nk[vb];
#pragma unroll 1
      for (int m = t; m < mc; m += TRK_THREADS) {
        const int2 r = rows[(long)p * M + m];
        if (!((unsigned)r.x < ka && (unsigned)r.y < kb)) continue;
        const int lu = trk_label(lab, va * K + r.x), lv = trk_label(lab, vb * K + r.y);
        if (lu != lv) {
          atomicMin(&lab[max(lu, lv)], min(lu, lv));
          hooked = 1;
        }
      }
    }
    if (!__syncthreads_or(hooked)) break;
#pragma unroll 1
    for (int pass = 0; pass < 32; ++pass) {
      int moved = 0;
#pragma unroll 1
      for (int u = t; u < n; u += TRK_THREADS) {
        const int p = trk_label(lab, u), g = trk_label(lab, p);
        if (g != p) {
          lab[u] = g;
          moved = 1;
        }
      }
      if (!__syncthreads_or(moved)) break;
    }
  }

  // views of every component, and the components that hold a view twice
#pragma unroll 1
  for (int v = 0; v < V; ++v) {
    const int kv = nk[v];
#pragma unroll 1
    for (int i = t; i < kv; i += TRK_THREADS) slot[trk_label(lab, v * K + i)] = v * K + i;
    __syncthreads();
#pragma unroll 1
    for (int i = t; i < kv; i += TRK_THREADS) {
      const int u = v * K + i, r = trk_label(lab, u);
      if (slot[r] == u) mask[r] |= 1 << v;  // one writer per root and view
      else conf[r] = 1;
    }
    __syncthreads();
  }

  // numbers: wave w walks the ids [w seg, (w + 1) seg), seg a multiple of 64
  const int wave = t >> 6, lane = t & 63;
  const int seg = ((n + TRK_WAVES - 1) / TRK_WAVES + 63) & ~63;
  const int lo = wave * seg, hi = min(n, lo + seg);
  int ntr = 0, ncomp = 0, ndrop = 0;
#pragma unroll 1
  for (int base = lo; base < hi; base += 64) {
    const int r = base + lane;
    bool root = false, bad = false;
    int nv = 0;
    if (r < hi && trk_label(lab, r) == r) {
      root = true;
      bad = conf[r] != 0;
      nv = __popc(mask[r]);
    }
    ntr += __popcll(__ballot(root && !bad && nv >= P.min_views));
    ncomp += __popcll(__ballot(root && (bad || nv >= 2)));
    ndrop += __popcll(__ballot(root && bad));
  }
  if (lane == 0) {
    wtot[0][wave] = ntr;
    wtot[1][wave] = ncomp;
    wtot[2][wave] = ndrop;
  }
  __syncthreads();
  int first = 0, total = 0, comps = 0, dropped = 0;
#pragma unroll
  for (int w = 0; w < TRK_WAVES; ++w) {
    first += w < wave ? wtot[0][w] : 0;
    total += wtot[0][w];
    comps += wtot[1][w];
    dropped += wtot[2][w];
  }
#pragma unroll 1
  for (int base = lo; base < hi; base += 64) {
    const int r = base + lane;
    const bool is = r < hi && trk_label(lab, r) == r && conf[r] == 0 && __popc(mask[r]) >= P.min_views;
    const unsigned long long bal = __ballot(is);
    if (r < hi) slot[r] = is ? first + wave_rank(bal) : -1;
    first += __popcll(bal);
  }

  // fill
  const int T = P.T;
  int* tracks = P.tracks + (long)b * V * T;
  float2* kp = P.kpts ? P.kpts + (long)b * V * T : nullptr;
  const float nanf_ = __int_as_float(0x7fc00000);
#pragma unroll 1
  for (long e = t; e < (long)V * T; e += TRK_THREADS) {
    tracks[e] = -1;
    if (kp) kp[e] = make_float2(nanf_, nanf_);
  }
  __syncthreads();
#pragma unroll 1
  for (int v = 0; v < V; ++v) {
    const int kv = nk[v];
#pragma unroll 1
    for (int i = t; i < kv; i += TRK_THREADS) {
      const int tn = slot[trk_label(lab, v * K + i)];
      if (tn >= 0 && tn < T) {
        tracks[(long)v * T + tn] = i;
        if (kp) kp[(long)v * T + tn] = P.x[((long)b * V + v) * K + i];
      }
    }
  }
  if (t == 0) {
    P.counts[b] = min(total, T);
    P.total[b] = total;
    int* row = P.info + (long)b * BUILD_TRACKS_INFO;
    row[0] = used;
    row[1] = ignored;
    row[2] = comps;
    row[3] = dropped;
  }
}

}  // namespace

extern "C" long roma_op_build_tracks_workspace(int B, int V, int K, int P, int M) {
  if (B <= 0 || V <= 0 || K <= 0 || V > ROMA_TRACKS_MAX_VIEWS || K > ROMA_TRACKS_MAX_KPTS) return 0;
  TrkParams T;
  return trk_carve(Workspace256(), B, V, K, T);
}

extern "C" int roma_op_build_tracks(const int* inds, const int* pair_views, const int* match_counts, const int* num_kpts, const float* x,
                                    int B, int V, int K, int Pn, int M, int T, int min_views, int* out_tracks, float* out_kpts,
                                    int* out_counts, int* out_total, int* out_info, void* ws, long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(out_tracks && out_counts && out_total && out_info, "build_tracks: null pointer");
  ROMA_REQUIRE(V >= 2 && V <= ROMA_TRACKS_MAX_VIEWS, "build_tracks: need 2 <= V <= 8 views");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "build_tracks: B must lie in [0, 65535]");
  ROMA_REQUIRE(K >= 0 && K <= ROMA_TRACKS_MAX_KPTS, "build_tracks: need 0 <= K <= 65536 keypoints per view");
  ROMA_REQUIRE(Pn >= 0 && Pn <= ROMA_TRACKS_MAX_PAIRS, "build_tracks: need 0 <= P <= 64 pairs");
  ROMA_REQUIRE(M >= 0 && T >= 0, "build_tracks: M and max_tracks must not be negative");
  ROMA_REQUIRE(min_views >= 2 && min_views <= V, "build_tracks: need 2 <= min_views <= V");
  ROMA_REQUIRE((x == nullptr) == (out_kpts == nullptr), "build_tracks: x and out_kpts go together");
  ROMA_REQUIRE(Pn == 0 || (pair_views && (M == 0 || inds)), "build_tracks: null pointer");
  ROMA_REQUIRE((long)B * Pn * M < (1l << 30) && (long)B * V * T < (1l << 30), "build_tracks: B * P * M and B * V * max_tracks must be below 2^30");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(inds) & 7) == 0 && (reinterpret_cast<uintptr_t>(x) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_kpts) & 7) == 0,
               "build_tracks: inds, x and out_kpts must be 8-byte aligned");
  TrkParams P = {};
  if (int rc = check_pairs("build_tracks", pair_views, V, Pn, P.pv.v)) return rc;  // whether or not a row will be read
  if (B == 0) return 0;
  ROMA_REQUIRE(K == 0 || (ws && ws_bytes >= (size_t)roma_op_build_tracks_workspace(B, V, K, Pn, M)), "build_tracks: workspace too small");
  P.inds = reinterpret_cast<const int2*>(inds);
  P.match_counts = match_counts;
  P.num_kpts = num_kpts;
  P.x = reinterpret_cast<const float2*>(x);
  P.V = V, P.K = K, P.P = M > 0 ? Pn : 0, P.M = M, P.T = T, P.min_views = min_views;
  P.tracks = out_tracks;
  P.kpts = reinterpret_cast<float2*>(out_kpts);
  P.counts = out_counts, P.total = out_total, P.info = out_info;
  trk_carve(Workspace256(ws), B, V, K, P);
  ProfScope ps("build_tracks_kernel", (double)B * ((double)Pn * M + (double)V * K), "B", s);
  hipLaunchKernelGGL(build_tracks_kernel, dim3(B), dim3(TRK_THREADS), 0, s, P);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
