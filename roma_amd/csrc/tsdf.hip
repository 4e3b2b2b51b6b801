// Truncated signed distance volumes: roma_op_tsdf_integrate adds depth maps to a volume, roma_op_tsdf_extract_mesh turns its zero
// level set into a triangle mesh by marching tetrahedra, roma_op_points_bounds sizes a volume from a cloud.  The definitions are in
// include/roma_hip_tsdf.h; tools/tsdf_ref.py restates them in numpy - float64 where the device is float64, float32 operation by
// operation where it is float32 - and is the oracle of tests/test_gpu_tsdf.py.
//
// Integration: one thread per voxel, x fastest, so a wave reads and writes 256 contiguous bytes of tsdf and of weight; the V views
// of the problem are staged once per workgroup in LDS and taken in view order; the voxel's state is loaded once, updated in
// registers and stored once - and not stored at all where no view touched it.  The voxel centre is projected in float64 by the
// formula of the header, with no incremental form along x: the restatement is held to every bit, and a voxel's result must not
// depend on where its row started.
//
// Extraction is count -> scan -> emit over the grid points, one thread each, grid (blocks of 256 grid points, problem):
//   count    the 7-bit mask of the edges a grid point owns that carry a vertex, and the triangles of its cell: one byte per grid
//            point, two counts per block
//   scan     one workgroup per problem: the exclusive prefixes of both block counts in block order, counts, totals
//   vertex   the number of a grid point's first vertex is its block's prefix plus the scan of the mask populations inside the
//            block; it is kept per grid point, so that a face finds the vertex of edge class c of grid point q without a search, as
//            base[q] + popcount(mask[q] & ((1 << (c - 1)) - 1)); positions, colours, normals and the padding are written
//   face     the same for the triangles of a cell; a vertex's first use clears its rim flag
// Every phase is closed by a kernel boundary.  The only atomics are integer: the counters of `stats`, one per workgroup that has
// something to count, the exchange that finds a vertex's first use, and the minimum / maximum of roma_op_points_bounds.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip_tsdf.h"
#include "common.h"
#include "workgroup.h"
#include "workspace.h"

// nothing here is fused: tools/tsdf_ref.py evaluates the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int TSDF_MAX_VIEWS = 8;
constexpr int TSDF_MAX_COLOR_VIEWS = 128;  // B * V with a colour source: offsets and sizes travel in the kernel's arguments
constexpr int TSDF_STATS = 8;              // ints per problem in roma_op_tsdf_extract_mesh's out_stats
constexpr int TSDF_BLOCK = 256, TSDF_WAVES = TSDF_BLOCK / WAVE;
constexpr int TSDF_SCAN = 1024, TSDF_SCAN_WAVES = TSDF_SCAN / WAVE;
constexpr int BOUNDS_MAX_BLOCKS = 1024;  // per problem: each strides over the rows

struct TsdfParams {
  const float* depth;
  const float* dw;
  const double* cam;
  const double* R;
  const double* t;
  const unsigned char* view_valid;
  const unsigned char* valid;
  const double* origin;
  const double* voxel;
  const double* trunc;
  int B, V, H, W, nz, ny, nx;
  double near;
  float max_weight;
  float* tsdf;
  float* weight;
  float* color;
};

struct TsdfColors {  // the colour source: host data, in the kernel's arguments
  const unsigned char* images;
  long long offset[TSDF_MAX_COLOR_VIEWS];
  int h[TSDF_MAX_COLOR_VIEWS], w[TSDF_MAX_COLOR_VIEWS];
};

struct TView {
  double fx, fy, cx, cy, r[9], t[3];
  int on;
};

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_integrate_kernel(const TsdfParams P, const TsdfColors C) {
  __shared__ TView sv[TSDF_MAX_VIEWS];
  const int b = blockIdx.y;
  if ((int)threadIdx.x < P.V) {
    const int u = threadIdx.x;
    const long at = (long)b * P.V + u;
    const double* k = P.cam + at * 9;
    TView w;
    w.fx = k[0], w.fy = k[4], w.cx = k[2], w.cy = k[5];
#pragma unroll
    for (int i = 0; i < 9; ++i) w.r[i] = P.R[at * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) w.t[i] = P.t[at * 3 + i];
    w.on = !P.view_valid || P.view_valid[at] != 0 ? 1 : 0;
    sv[u] = w;
  }
  __syncthreads();
  const double vs = P.voxel[b], trunc = P.trunc[b];
  if ((P.valid && P.valid[b] == 0) || !(vs > 0.0) || !(trunc > 0.0)) return;  // NaN fails: the problem is left alone
  const int G = P.nz * P.ny * P.nx;
  const int n = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (n >= G) return;
  const int i = n % P.nx, jk = n / P.nx, j = jk % P.ny, k = jk / P.ny;
  const double X0 = P.origin[b * 3 + 0] + ((double)i + 0.5) * vs;
  const double X1 = P.origin[b * 3 + 1] + ((double)j + 0.5) * vs;
  const double X2 = P.origin[b * 3 + 2] + ((double)k + 0.5) * vs;
  const long at = (long)b * G + n;
  float T = P.tsdf[at], Wt = P.weight[at];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  if (P.color) c0 = P.color[at * 3 + 0], c1 = P.color[at * 3 + 1], c2 = P.color[at * 3 + 2];
  bool touched = false;
  const long npx = (long)P.H * P.W;
#pragma unroll 1
  for (int v = 0; v < P.V; ++v) {
    const TView& a = sv[v];
    if (!a.on) continue;
    const double y0 = ((a.r[0] * X0 + a.r[1] * X1) + a.r[2] * X2) + a.t[0];
    const double y1 = ((a.r[3] * X0 + a.r[4] * X1) + a.r[5] * X2) + a.t[1];
    const double z = ((a.r[6] * X0 + a.r[7] * X1) + a.r[8] * X2) + a.t[2];
    if (!(z > P.near)) continue;
    const double fu = floor(a.fx * (y0 / z) + a.cx), fv = floor(a.fy * (y1 / z) + a.cy);
    // in or out of the grid is decided in double, before any conversion to an integer; NaN fails
    if (!(fu >= 0.0 && fu < (double)P.W && fv >= 0.0 && fv < (double)P.H)) continue;
    const int c = (int)fu, r = (int)fv;
    const long px = ((long)b * P.V + v) * npx + ((long)r * P.W + c);
    const float d = P.depth[px];
    if (!(isfinite(d) && d > 0.0f)) continue;
    const float w = P.dw ? P.dw[px] : 1.0f;
    if (!(isfinite(w) && w > 0.0f)) continue;
    const double sdf = (double)d - z;
    if (sdf < -trunc) continue;
    const double q = sdf / trunc;
    const float f = (float)(q < 1.0 ? q : 1.0);
    const float den = Wt + w;
    T = (Wt * T + w * f) / den;
    if (P.color && sdf <= trunc) {
      // the image pixel that holds the centre of the cell: floor((c + 0.5) W_img / W) in integers
      const int cv = b * P.V + v;
      const long ix = ((2l * c + 1) * C.w[cv]) / (2l * P.W), iy = ((2l * r + 1) * C.h[cv]) / (2l * P.H);
      const unsigned char* rgb = C.images + C.offset[cv] + (iy * C.w[cv] + ix) * 3;
      c0 = (Wt * c0 + w * (float)rgb[0]) / den;
      c1 = (Wt * c1 + w * (float)rgb[1]) / den;
      c2 = (Wt * c2 + w * (float)rgb[2]) / den;
    }
    Wt = den < P.max_weight ? den : P.max_weight;
    touched = true;
  }
  if (!touched) return;
  P.tsdf[at] = T;
  P.weight[at] = Wt;
  if (P.color) P.color[at * 3 + 0] = c0, P.color[at * 3 + 1] = c1, P.color[at * 3 + 2] = c2;
}

// ------------------------------------------------------------------------------------------------------------------ extraction
struct MeshParams {
  const float* tsdf;
  const float* weight;
  const float* color;
  const unsigned char* valid;
  const double* origin;
  const double* voxel;
  int B, nz, ny, nx, G, nb;
  float min_weight;
  int max_v, max_f;
  float* verts;
  float* normals;
  unsigned char* colors;
  int* faces;
  int* counts;
  int* totals;
  int* stats;
  unsigned char* mask;  // [B, G] workspace: bit c - 1: the edge of class c carries a vertex
  int* base;            // [B, G] workspace: the number of the grid point's first vertex
  int* vsum;            // [B, nb] workspace: vertices of a block, then their exclusive prefix
  int* fsum;            // [B, nb] workspace: the same for faces
  unsigned* used;       // [B, max_v] workspace: 1 once a triangle names the vertex
};

// The Kuhn split.  Tetrahedron tau of a cell has the corners p + o[0 .. 3], o = 0, e_a, e_a + e_b, (1, 1, 1) as bit sets of the
// axes (x = 1, y = 2, z = 4), over the permutations (a, b, c) in lexicographic order; det(e_a, e_b, e_c) is its orientation.  Every
// edge of it runs from a corner to a later one, whose bit set contains the earlier one's: the edge is owned by grid point
// p + o[m] and its class is o[n] ^ o[m].  A face diagonal of the cube is the same segment in the cell beyond it (o is a
// translate), so the split is conforming.
__constant__ unsigned char TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ unsigned char TET_ODD[6] = {0, 1, 1, 0, 0, 1};
// Edges of a tetrahedron: 0 = 01, 1 = 02, 2 = 03, 3 = 12, 4 = 13, 5 = 23.
__constant__ unsigned char EDGE_END[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// The 16 cases, for a positively oriented tetrahedron (an odd one swaps the last two vertices of every triangle); bit n of the
// case: corner n is inside.  With (i, j, k, l) an EVEN permutation of the corners:
//   one corner i inside         the triangle (ij, ik, il): on 0, x, y, z with 0 inside it is (s, 0, 0), (0, s, 0), (0, 0, s), whose
//                               normal s^2 (1, 1, 1) points away from the inside corner
//   one corner i outside        the same triangle turned round, (ij, il, ik)
//   i < j inside, k, l outside  the quadrilateral (ik, il, jl, jk), cut along ik - jl: on 0, x inside and y, z outside it is
//                               (0, s, 0), (0, 0, s), (1 - s, 0, s), (1 - s, s, 0) with normal along (0, 1, 1), towards the outside pair
// tools/tsdf_ref.py derives the table from this rule and tests/test_cpu_tsdf.py compares the two.
__constant__ unsigned char TET_NTRI[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__constant__ unsigned char TET_TRI[16][6] = {
    {0, 0, 0, 0, 0, 0}, {0, 1, 2, 0, 0, 0}, {0, 4, 3, 0, 0, 0}, {1, 2, 4, 1, 4, 3}, {1, 3, 5, 0, 0, 0}, {2, 0, 3, 2, 3, 5},
    {0, 4, 5, 0, 5, 1}, {2, 4, 5, 0, 0, 0}, {2, 5, 4, 0, 0, 0}, {0, 1, 5, 0, 5, 4}, {3, 0, 2, 3, 2, 5}, {1, 5, 3, 0, 0, 0},
    {1, 3, 4, 1, 4, 2}, {0, 3, 4, 0, 0, 0}, {0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};

__device__ __forceinline__ bool mesh_problem_on(const MeshParams& P, int b) {
  return (!P.valid || P.valid[b] != 0) && P.voxel[b] > 0.0;
}

// valid and inside of the 8 corners p + o of the cell at grid point (i, j, k), bit o each; a corner outside the grid is not valid
__device__ __forceinline__ void mesh_corner_bits(const MeshParams& P, long vol, int i, int j, int k, unsigned& vb, unsigned& ib) {
  vb = 0, ib = 0;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int ii = i + (o & 1), jj = j + ((o >> 1) & 1), kk = k + (o >> 2);
    if (ii < P.nx && jj < P.ny && kk < P.nz) {
      const long at = vol + ((long)kk * P.ny + jj) * P.nx + ii;
      if (P.weight[at] >= P.min_weight) {  // NaN fails
        vb |= 1u << o;
        if (P.tsdf[at] < 0.0f) ib |= 1u << o;
      }
    }
  }
}

// the mask of the edges that grid point owns and that carry a vertex
__device__ __forceinline__ unsigned mesh_edge_mask(unsigned vb, unsigned ib) {
  unsigned m = 0;
  if (vb & 1u) {
#pragma unroll
    for (int c = 1; c < 8; ++c)
      if (((vb >> c) & 1u) && (((ib >> c) ^ ib) & 1u)) m |= 1u << (c - 1);
  }
  return m;
}

// the inside bits of the four corners of tetrahedron tau, or -1 when a corner is not valid
__device__ __forceinline__ int mesh_tet_case(unsigned vb, unsigned ib, int tau) {
  int m = 0;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int o = TET_CORNER[tau][n];
    if (!((vb >> o) & 1u)) return -1;
    m |= (int)((ib >> o) & 1u) << n;
  }
  return m;
}

__device__ __forceinline__ int mesh_cell_faces(unsigned vb, unsigned ib) {
  int nf = 0;
#pragma unroll
  for (int tau = 0; tau < 6; ++tau) {
    const int m = mesh_tet_case(vb, ib, tau);
    if (m >= 0) nf += TET_NTRI[m];
  }
  return nf;
}

__global__ __launch_bounds__(TSDF_BLOCK) void mesh_count_kernel(const MeshParams P) {
  __shared__ int sh[TSDF_WAVES];
  const int b = blockIdx.y, n = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  const bool in = n < P.G && mesh_problem_on(P, b);
  unsigned vb = 0, ib = 0;
  if (in) {
    const int i = n % P.nx, jk = n / P.nx;
    mesh_corner_bits(P, (long)b * P.G, i, jk % P.ny, jk / P.ny, vb, ib);
  }
  const unsigned m = mesh_edge_mask(vb, ib);
  const int nf = mesh_cell_faces(vb, ib);
  if (n < P.G) P.mask[(long)b * P.G + n] = (unsigned char)m;
  const int nv_block = wg_sum<TSDF_WAVES>(__popc(m), sh);
  const int nf_block = wg_sum<TSDF_WAVES>(nf, sh);
  if (threadIdx.x == 0) {
    P.vsum[(long)b * P.nb + blockIdx.x] = nv_block;
    P.fsum[(long)b * P.nb + blockIdx.x] = nf_block;
  }
  __syncthreads();  // wg_sum's readers are done with sh
  int* stats = P.stats + (long)b * TSDF_STATS;
  wg_count_add<TSDF_WAVES>(stats + 0, (vb & 1u) != 0, sh);
  wg_count_add<TSDF_WAVES>(stats + 1, (vb & ib & 1u) != 0, sh);
  wg_count_add<TSDF_WAVES>(stats + 6, nf > 0, sh);
}

// one workgroup per problem: vsum and fsum become their own exclusive prefixes in block order
__global__ __launch_bounds__(TSDF_SCAN) void mesh_scan_kernel(const MeshParams P) {
  __shared__ int wt[TSDF_SCAN_WAVES];
  const int b = blockIdx.x, t = threadIdx.x;
  const int per = (P.nb + TSDF_SCAN - 1) / TSDF_SCAN;
  const int lo = std::min(t * per, P.nb), hi = std::min(lo + per, P.nb);
  int sums[2];
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    int* bs = (which ? P.fsum : P.vsum) + (long)b * P.nb;
    int mine = 0;
#pragma unroll 1
    for (int i = lo; i < hi; ++i) mine += bs[i];
    int sum;
    int before = wg_scan_exclusive<TSDF_SCAN_WAVES>(mine, wt, sum);
#pragma unroll 1
    for (int i = lo; i < hi; ++i) {
      const int cnt = bs[i];
      bs[i] = before;
      before += cnt;
    }
    sums[which] = sum;
  }
  if (t == 0) {
    const int nv = std::min(sums[0], P.max_v), nf = std::min(sums[1], P.max_f);
    P.totals[b * 2 + 0] = sums[0], P.totals[b * 2 + 1] = sums[1];
    P.counts[b * 2 + 0] = nv, P.counts[b * 2 + 1] = nf;
    int* stats = P.stats + (long)b * TSDF_STATS;
    stats[2] = nv, stats[3] = nf;
    stats[4] = nv;  // every written vertex is on the rim until a triangle names it
  }
}

// the central differences of tsdf at grid point (i, j, k): false when one of the six neighbours is outside the grid or not valid
__device__ __forceinline__ bool mesh_gradient(const MeshParams& P, long vol, int i, int j, int k, double (&g)[3]) {
  if (i < 1 || j < 1 || k < 1 || i > P.nx - 2 || j > P.ny - 2 || k > P.nz - 2) return false;
  const long at = vol + ((long)k * P.ny + j) * P.nx + i;
  const long step[3] = {1l, (long)P.nx, (long)P.nx * P.ny};
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ok = ok && P.weight[at + step[a]] >= P.min_weight && P.weight[at - step[a]] >= P.min_weight;
    g[a] = (double)P.tsdf[at + step[a]] - (double)P.tsdf[at - step[a]];
  }
  return ok;
}

__global__ __launch_bounds__(TSDF_BLOCK) void mesh_vertex_kernel(const MeshParams P) {
  __shared__ int wt[TSDF_WAVES];
  const int b = blockIdx.y, n = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  const long vol = (long)b * P.G;
  const unsigned m = n < P.G ? P.mask[vol + n] : 0u;
  int in_block_total;
  const int first = P.vsum[(long)b * P.nb + blockIdx.x] + wg_scan_exclusive<TSDF_WAVES>((int)__popc(m), wt, in_block_total);
  if (n < P.G) P.base[vol + n] = first;
  const float nanf_ = __int_as_float(0x7fc00000);
  const long rows = (long)b * P.max_v;
  if (m) {
    const int i = n % P.nx, jk = n / P.nx, j = jk % P.ny, k = jk / P.ny;
    const double vs = P.voxel[b];
    const double f0 = (double)P.tsdf[vol + n];
    double g0[3] = {0.0, 0.0, 0.0};
    const bool have0 = mesh_gradient(P, vol, i, j, k, g0);
    int idx = first;
#pragma unroll 1
    for (int c = 1; c < 8; ++c) {
      if (!((m >> (c - 1)) & 1u)) continue;
      const int at_v = idx++;
      if (at_v >= P.max_v) break;
      const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
      const long far = vol + ((long)(k + dz) * P.ny + (j + dy)) * P.nx + (i + dx);
      const double f1 = (double)P.tsdf[far];
      const double s = f0 / (f0 - f1);  // exactly one end is below 0: the difference is not 0
      float* xyz = P.verts + (rows + at_v) * 3;
      xyz[0] = (float)(P.origin[b * 3 + 0] + (((double)i + 0.5) + s * (double)dx) * vs);
      xyz[1] = (float)(P.origin[b * 3 + 1] + (((double)j + 0.5) + s * (double)dy) * vs);
      xyz[2] = (float)(P.origin[b * 3 + 2] + (((double)k + 0.5) + s * (double)dz) * vs);
      double g1[3] = {0.0, 0.0, 0.0};
      const bool have = mesh_gradient(P, vol, i + dx, j + dy, k + dz, g1) && have0;
      const double gx = g0[0] + s * (g1[0] - g0[0]), gy = g0[1] + s * (g1[1] - g0[1]), gz = g0[2] + s * (g1[2] - g0[2]);
      const double len = sqrt((gx * gx + gy * gy) + gz * gz);
      float* nrm = P.normals + (rows + at_v) * 3;
      if (have && len > 0.0) {
        nrm[0] = (float)(gx / len), nrm[1] = (float)(gy / len), nrm[2] = (float)(gz / len);
      } else {
        nrm[0] = nanf_, nrm[1] = nanf_, nrm[2] = nanf_;
      }
      if (P.colors) {
        unsigned char* rgb = P.colors + (rows + at_v) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const double a0 = (double)P.color[(vol + n) * 3 + ch], a1 = (double)P.color[far * 3 + ch];
          double v = a0 + s * (a1 - a0);
          v = v > 0.0 ? v : 0.0;  // NaN becomes 0
          v = v < 255.0 ? v : 255.0;
          rgb[ch] = (unsigned char)(int)floor(v + 0.5);
        }
      }
    }
  }
  // the padding beyond the vertices, by the threads of the whole problem
  const long begin = P.counts[b * 2 + 0], step = (long)P.nb * TSDF_BLOCK;
#pragma unroll 1
  for (long r = begin + (long)blockIdx.x * TSDF_BLOCK + threadIdx.x; r < P.max_v; r += step) {
    float* xyz = P.verts + (rows + r) * 3;
    float* nrm = P.normals + (rows + r) * 3;
    xyz[0] = nanf_, xyz[1] = nanf_, xyz[2] = nanf_;
    nrm[0] = nanf_, nrm[1] = nanf_, nrm[2] = nanf_;
    if (P.colors) {
      unsigned char* rgb = P.colors + (rows + r) * 3;
      rgb[0] = 0, rgb[1] = 0, rgb[2] = 0;
    }
  }
}

__global__ __launch_bounds__(TSDF_BLOCK) void mesh_face_kernel(const MeshParams P) {
  __shared__ int wt[TSDF_WAVES];
  const int b = blockIdx.y, n = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  const long vol = (long)b * P.G;
  const bool in = n < P.G && mesh_problem_on(P, b);
  const int i = n % P.nx, jk = n / P.nx, j = jk % P.ny, k = jk / P.ny;
  unsigned vb = 0, ib = 0;
  if (in) mesh_corner_bits(P, vol, i, j, k, vb, ib);
  const int nf = mesh_cell_faces(vb, ib);
  int in_block_total;
  int f = P.fsum[(long)b * P.nb + blockIdx.x] + wg_scan_exclusive<TSDF_WAVES>(nf, wt, in_block_total);
  const long rows = (long)b * P.max_f;
  int first_uses = 0, cut = 0;
  if (nf) {
#pragma unroll 1
    for (int tau = 0; tau < 6; ++tau) {
      const int m = mesh_tet_case(vb, ib, tau);
      if (m < 0) continue;
#pragma unroll 1
      for (int tri = 0; tri < TET_NTRI[m]; ++tri, ++f) {
        int vn[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const int edge = TET_TRI[m][tri * 3 + e];
          const int oa = TET_CORNER[tau][EDGE_END[edge][0]], c = oa ^ TET_CORNER[tau][EDGE_END[edge][1]];
          const long q = vol + ((long)(k + (oa >> 2)) * P.ny + (j + ((oa >> 1) & 1))) * P.nx + (i + (oa & 1));
          vn[e] = P.base[q] + __popc((unsigned)P.mask[q] & ((1u << (c - 1)) - 1u));
        }
        if (TET_ODD[tau]) {
          const int swap = vn[1];
          vn[1] = vn[2], vn[2] = swap;
        }
        bool whole = true;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          if (vn[e] < P.max_v) {
            unsigned* u = P.used + (long)b * P.max_v + vn[e];
            // a flag only ever goes from 0 to 1, so a plain look first is exact: a stale 0 costs an exchange that was not needed
            if (__hip_atomic_load(u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && atomicExch(u, 1u) == 0u) ++first_uses;
          } else {
            whole = false;
          }
        }
        if (f < P.max_f) {
          int* row = P.faces + (rows + f) * 3;
          row[0] = whole ? vn[0] : -1, row[1] = whole ? vn[1] : -1, row[2] = whole ? vn[2] : -1;
          cut += whole ? 0 : 1;
        }
      }
    }
  }
  int* stats = P.stats + (long)b * TSDF_STATS;
  const int uses = wg_sum<TSDF_WAVES>(first_uses, wt), cuts = wg_sum<TSDF_WAVES>(cut, wt);
  if (threadIdx.x == 0) {
    if (uses) atomicSub(stats + 4, uses);
    if (cuts) atomicAdd(stats + 5, cuts);
  }
  // the padding beyond the faces, by the threads of the whole problem
  const long begin = P.counts[b * 2 + 1], step = (long)P.nb * TSDF_BLOCK;
#pragma unroll 1
  for (long r = begin + (long)blockIdx.x * TSDF_BLOCK + threadIdx.x; r < P.max_f; r += step) {
    int* row = P.faces + (rows + r) * 3;
    row[0] = -1, row[1] = -1, row[2] = -1;
  }
}

// B nz ny nx < 2^31 and 7 nz ny nx < 2^31, by divisions: the products themselves may not fit
bool volume_ok(int B, int nz, int ny, int nx) {
  if (B < 1 || nz < 1 || ny < 1 || nx < 1) return false;
  const long lim = (1l << 31) - 1, per = std::max<long>(B, 7);
  return (long)ny * nx <= lim / nz && (long)nz * ny * nx <= lim / per;
}

size_t mesh_carve(Workspace256 ws, int B, int nz, int ny, int nx, int max_v, MeshParams& P) {
  const size_t G = (size_t)nz * ny * nx, nb = (G + TSDF_BLOCK - 1) / TSDF_BLOCK;
  P.mask = ws.take<unsigned char>(B * G);
  P.base = ws.take<int>(B * G);
  P.vsum = ws.take<int>(B * nb);
  P.fsum = ws.take<int>(B * nb);
  P.used = ws.take<unsigned>((size_t)B * max_v);
  return ws.bytes();
}

// ---------------------------------------------------------------------------------------------------------------------- bounds
struct BoundsParams {
  const float* points;
  const int* counts;
  int B, N, nb;
  unsigned* kmin;  // [B, 3] workspace, all ones on entry
  unsigned* kmax;  // [B, 3] workspace, 0 on entry
  int* ticket;     // [B] workspace, 0 on entry: the blocks of the problem that are done
  double* out;
};

// the order of the finite floats as unsigned integers; never 0 and never all ones
__device__ __forceinline__ unsigned bounds_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bounds_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

__global__ __launch_bounds__(TSDF_BLOCK) void points_bounds_kernel(const BoundsParams Q) {
  __shared__ unsigned sh[6][TSDF_WAVES];
  const int b = blockIdx.y;
  int cnt = Q.N;
  if (Q.counts) {
    const int given = Q.counts[b];
    cnt = given < 0 ? 0 : given < Q.N ? given : Q.N;
  }
  unsigned k[6] = {~0u, ~0u, ~0u, 0u, 0u, 0u};
#pragma unroll 1
  for (long n = (long)blockIdx.x * TSDF_BLOCK + threadIdx.x; n < cnt; n += (long)Q.nb * TSDF_BLOCK) {
    const float* p = Q.points + ((long)b * Q.N + n) * 3;
    const float x0 = p[0], x1 = p[1], x2 = p[2];
    if (isfinite(x0) && isfinite(x1) && isfinite(x2)) {
      const unsigned a0 = bounds_key(x0), a1 = bounds_key(x1), a2 = bounds_key(x2);
      k[0] = min(k[0], a0), k[1] = min(k[1], a1), k[2] = min(k[2], a2);
      k[3] = max(k[3], a0), k[4] = max(k[4], a1), k[5] = max(k[5], a2);
    }
  }
#pragma unroll
  for (int off = WAVE / 2; off >= 1; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      k[a] = min(k[a], (unsigned)__shfl_xor((int)k[a], off));
      k[3 + a] = max(k[3 + a], (unsigned)__shfl_xor((int)k[3 + a], off));
    }
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) sh[a][threadIdx.x / WAVE] = k[a];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      unsigned lo = ~0u, hi = 0u;
#pragma unroll
      for (int w = 0; w < TSDF_WAVES; ++w) lo = min(lo, sh[a][w]), hi = max(hi, sh[3 + a][w]);
      if (lo != ~0u) atomicMin(Q.kmin + b * 3 + a, lo);
      if (hi != 0u) atomicMax(Q.kmax + b * 3 + a, hi);
    }
    __threadfence();  // the minima and maxima of this block are visible before its ticket is
    if (atomicAdd(Q.ticket + b, 1) == Q.nb - 1) {  // the last block of the problem writes the result
      __threadfence();
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const unsigned lo = __hip_atomic_load(Q.kmin + b * 3 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned hi = __hip_atomic_load(Q.kmax + b * 3 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double nan_ = __longlong_as_double(0x7ff8000000000000ll);
        Q.out[b * 6 + a] = lo != ~0u ? (double)bounds_value(lo) : nan_;
        Q.out[b * 6 + 3 + a] = hi != 0u ? (double)bounds_value(hi) : nan_;
      }
    }
  }
}

size_t bounds_carve(Workspace256 ws, int B, BoundsParams& Q) {
  Q.kmin = ws.take<unsigned>((size_t)B * 3);
  Q.kmax = ws.take<unsigned>((size_t)B * 3);
  Q.ticket = ws.take<int>((size_t)B);
  return ws.bytes();
}

}  // namespace

extern "C" int roma_op_tsdf_integrate(const float* depth, const float* depth_weight, const double* cameras, const double* R,
                                      const double* t, const unsigned char* view_valid, const unsigned char* valid,
                                      const unsigned char* images, const long long* image_offsets, const int* image_sizes,
                                      const double* origin, const double* voxel_size, const double* trunc, int B, int V, int H, int W,
                                      int nz, int ny, int nx, float max_weight, double near, float* tsdf, float* weight, float* color,
                                      void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(depth && cameras && R && t && origin && voxel_size && trunc && tsdf && weight, "tsdf_integrate: null pointer");
  ROMA_REQUIRE(V >= 1 && V <= TSDF_MAX_VIEWS, "tsdf_integrate: need 1 <= V <= 8 views a call");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "tsdf_integrate: B must lie in [0, 65535]");
  ROMA_REQUIRE(H >= 1 && W >= 1, "tsdf_integrate: H and W must be positive");
  ROMA_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, "tsdf_integrate: nz, ny and nx must be positive");
  ROMA_REQUIRE(max_weight > 0.0f, "tsdf_integrate: max_weight must be positive");
  ROMA_REQUIRE(near >= 0.0, "tsdf_integrate: near is negative (or NaN)");
  ROMA_REQUIRE((images != nullptr) == (image_offsets != nullptr) && (images != nullptr) == (image_sizes != nullptr),
               "tsdf_integrate: images, image_offsets and image_sizes go together");
  ROMA_REQUIRE((images != nullptr) == (color != nullptr), "tsdf_integrate: color and the colour source go together");
  if (B == 0) return 0;
  ROMA_REQUIRE(volume_ok(B, nz, ny, nx), "tsdf_integrate: B * nz * ny * nx and 7 * nz * ny * nx must be below 2^31");
  ROMA_REQUIRE(W <= (1 << 30) && (long)H * W < (1l << 31) / ((long)B * V), "tsdf_integrate: B * V * H * W must be below 2^31");
  TsdfColors C = {};
  if (color) {
    ROMA_REQUIRE(B * V <= TSDF_MAX_COLOR_VIEWS, "tsdf_integrate: with a colour source B * V must not exceed 128");
    for (int k = 0; k < B * V; ++k) {
      ROMA_REQUIRE(image_sizes[2 * k] >= 1 && image_sizes[2 * k + 1] >= 1 && image_offsets[k] >= 0,
                   "tsdf_integrate: image sizes must be positive and image offsets not negative");
      C.offset[k] = image_offsets[k], C.h[k] = image_sizes[2 * k], C.w[k] = image_sizes[2 * k + 1];
    }
    C.images = images;
  }
  TsdfParams P = {};
  P.depth = depth, P.dw = depth_weight, P.cam = cameras, P.R = R, P.t = t, P.view_valid = view_valid, P.valid = valid;
  P.origin = origin, P.voxel = voxel_size, P.trunc = trunc;
  P.B = B, P.V = V, P.H = H, P.W = W, P.nz = nz, P.ny = ny, P.nx = nx;
  P.near = near, P.max_weight = max_weight;
  P.tsdf = tsdf, P.weight = weight, P.color = color;
  const long G = (long)nz * ny * nx;
  // the bytes a sweep moves when every voxel is touched: tsdf and weight (and colour) read and written; the depth maps stay in cache
  ProfScope ps("tsdf_integrate_kernel", (double)B * (double)G * (color ? 40.0 : 16.0), "B", s);
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((G + TSDF_BLOCK - 1) / TSDF_BLOCK), B), dim3(TSDF_BLOCK), 0, s, P, C);
  ROMA_LAUNCH_CHECK();
  return 0;
}

extern "C" long roma_op_tsdf_extract_mesh_workspace(int B, int nz, int ny, int nx, int max_vertices) {
  if (!volume_ok(B, nz, ny, nx) || B > 65535 || max_vertices < 0 || (long)max_vertices >= (1l << 31) / (3l * B)) return 0;
  MeshParams P;
  return mesh_carve(Workspace256(), B, nz, ny, nx, max_vertices, P);
}

extern "C" int roma_op_tsdf_extract_mesh(const float* tsdf, const float* weight, const float* color, const unsigned char* valid,
                                         const double* origin, const double* voxel_size, int B, int nz, int ny, int nx,
                                         float min_weight, int max_vertices, int max_faces, float* out_vertices, float* out_normals,
                                         unsigned char* out_colors, int* out_faces, int* out_counts, int* out_totals, int* out_stats,
                                         void* ws, long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(tsdf && weight && origin && voxel_size, "tsdf_extract_mesh: null pointer");
  ROMA_REQUIRE(out_vertices && out_normals && out_faces && out_counts && out_totals && out_stats, "tsdf_extract_mesh: null pointer");
  ROMA_REQUIRE((color != nullptr) == (out_colors != nullptr), "tsdf_extract_mesh: color and out_colors go together");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "tsdf_extract_mesh: B must lie in [0, 65535]");
  ROMA_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, "tsdf_extract_mesh: nz, ny and nx must be positive");
  ROMA_REQUIRE(min_weight > 0.0f, "tsdf_extract_mesh: min_weight must be positive (a voxel of weight 0 holds nothing)");
  ROMA_REQUIRE(max_vertices >= 0 && max_faces >= 0, "tsdf_extract_mesh: max_vertices and max_faces must not be negative");
  if (B == 0) return 0;
  ROMA_REQUIRE(volume_ok(B, nz, ny, nx), "tsdf_extract_mesh: B * nz * ny * nx and 7 * nz * ny * nx must be below 2^31");
  ROMA_REQUIRE((long)max_vertices < (1l << 31) / (3l * B) && (long)max_faces < (1l << 31) / (3l * B),
               "tsdf_extract_mesh: 3 * B * max_vertices and 3 * B * max_faces must be below 2^31");
  ROMA_REQUIRE(ws && ws_bytes >= (size_t)roma_op_tsdf_extract_mesh_workspace(B, nz, ny, nx, max_vertices),
               "tsdf_extract_mesh: workspace too small");
  MeshParams P = {};
  mesh_carve(Workspace256(ws), B, nz, ny, nx, max_vertices, P);
  P.tsdf = tsdf, P.weight = weight, P.color = color, P.valid = valid, P.origin = origin, P.voxel = voxel_size;
  P.B = B, P.nz = nz, P.ny = ny, P.nx = nx, P.G = nz * ny * nx, P.nb = (P.G + TSDF_BLOCK - 1) / TSDF_BLOCK;
  P.min_weight = min_weight, P.max_v = max_vertices, P.max_f = max_faces;
  P.verts = out_vertices, P.normals = out_normals, P.colors = out_colors, P.faces = out_faces;
  P.counts = out_counts, P.totals = out_totals, P.stats = out_stats;
  const double grid_points = (double)B * P.G;
  {
    ProfScope ps("mesh_clear", (double)B * max_vertices * 4.0, "B", s);
    ROMA_CHECK_HIP(hipMemsetAsync(out_stats, 0, (size_t)B * TSDF_STATS * sizeof(int), s));
    if (max_vertices > 0) ROMA_CHECK_HIP(hipMemsetAsync(P.used, 0, (size_t)B * max_vertices * sizeof(unsigned), s));
  }
  const dim3 grid(P.nb, B);
  {
    ProfScope ps("mesh_count_kernel", grid_points * 9.0, "B", s);
    hipLaunchKernelGGL(mesh_count_kernel, grid, dim3(TSDF_BLOCK), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("mesh_scan_kernel", (double)B * P.nb * 16.0, "B", s);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(B), dim3(TSDF_SCAN), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("mesh_vertex_kernel", grid_points * 5.0 + (double)B * max_vertices * (color ? 27.0 : 24.0), "B", s);
    hipLaunchKernelGGL(mesh_vertex_kernel, grid, dim3(TSDF_BLOCK), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("mesh_face_kernel", grid_points * 8.0 + (double)B * max_faces * 12.0, "B", s);
    hipLaunchKernelGGL(mesh_face_kernel, grid, dim3(TSDF_BLOCK), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" long roma_op_points_bounds_workspace(int B) {
  if (B < 1 || B > 65535) return 0;
  BoundsParams Q;
  return bounds_carve(Workspace256(), B, Q);
}

extern "C" int roma_op_points_bounds(const float* points, const int* counts, int B, int N, double* out, void* ws, long workspace_bytes,
                                     void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = workspace_size(workspace_bytes);
  ROMA_REQUIRE(out, "points_bounds: null pointer");
  ROMA_REQUIRE(B >= 0 && B <= 65535, "points_bounds: B must lie in [0, 65535]");
  ROMA_REQUIRE(N >= 0, "points_bounds: N must not be negative");
  ROMA_REQUIRE(points || N == 0, "points_bounds: null pointer");
  if (B == 0) return 0;
  ROMA_REQUIRE((long)N < (1l << 31) / (3l * B), "points_bounds: 3 * B * N must be below 2^31");
  ROMA_REQUIRE(ws && ws_bytes >= (size_t)roma_op_points_bounds_workspace(B), "points_bounds: workspace too small");
  BoundsParams Q = {};
  bounds_carve(Workspace256(ws), B, Q);
  Q.points = points, Q.counts = counts, Q.B = B, Q.N = N, Q.out = out;
  Q.nb = (int)std::min<long>(std::max<long>(((long)N + TSDF_BLOCK - 1) / TSDF_BLOCK, 1), BOUNDS_MAX_BLOCKS);
  ROMA_CHECK_HIP(hipMemsetAsync(Q.kmin, 0xFF, (size_t)B * 3 * sizeof(unsigned), s));
  ROMA_CHECK_HIP(hipMemsetAsync(Q.kmax, 0, (size_t)B * 3 * sizeof(unsigned), s));
  ROMA_CHECK_HIP(hipMemsetAsync(Q.ticket, 0, (size_t)B * sizeof(int), s));
  ProfScope ps("points_bounds_kernel", (double)B * N * 12.0, "B", s);
  hipLaunchKernelGGL(points_bounds_kernel, dim3(Q.nb, B), dim3(TSDF_BLOCK), 0, s, Q);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
