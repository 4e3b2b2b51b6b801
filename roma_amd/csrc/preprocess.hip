// Image preprocessing on the device (roma_op_preprocess): the 8-bit bicubic resize of Pillow's Image.resize(..., BICUBIC) for packed
// RGB images of mixed sizes, to one or two target sizes, followed by the / 255 and ImageNet normalisation of the matcher's host path
// (roma_amd/matcher.py: _pil_to_normalised).  The definition is stated in include/roma_hip.h and restated in numpy by
// tools/pil_resample_ref.py; every output bit equals the host path's.
//
// Pillow resamples in fixed point (22 fractional bits) in two passes, HORIZONTAL first, then VERTICAL, and rounds the intermediate
// image to uint8 between them; an axis whose size does not change is skipped.  Three kernels, one enqueue, nothing read back:
//   1. preprocess_coeff_kernel       the coefficient tables of every (image, target, axis) in float64 with contraction off, one
//                                    thread per output coordinate, and the 768-entry normalisation table;
//   2. preprocess_horizontal_kernel  packed uint8 rows -> uint8 [H_in, w_out, 3] intermediate (rows padded to whole dwords);
//   3. preprocess_vertical_kernel    intermediate (or the source, where the horizontal pass is skipped) -> float32 NCHW through the
//                                    normalisation table.
// Grids are (blocks, image, target), so sizes, offsets and table bases are wave-uniform; blocks are capped and stride over the work.
// The workspace is laid out from the LARGEST image of the host descriptors (equal slots per image), so the kernels find every slot
// from the image index alone; they read the sizes from the device descriptors and skip an image whose device descriptor does not fit
// what the host planned for (it can then never read or write out of bounds).
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "common.h"

// the coefficient arithmetic is evaluated as written: tools/pil_resample_ref.py has the same expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int PRE_THREADS = 256;
constexpr int PRE_MAX_BLOCKS = 2048;  // whole grid: 256 CUs x 8 workgroups; the rest is the block-stride loop
constexpr int PRECISION_BITS = 22;
constexpr int MAX_SIDE = 32768;
constexpr long NORM_BYTES = 768 * sizeof(float);

// horizontal pass: a workgroup makes 256 output bytes (64 dwords: one wave stores 256 contiguous bytes) of 16 rows at a time, from
// source pixels staged in LDS 64 at a time, with the coefficients that fall on them
constexpr int H_STRIP_BYTES = 256;
constexpr int H_STRIP_COLS = 87;  // pixels that touch 256 consecutive bytes: at most 86, + 1
constexpr int H_RG = 4;           // row groups of a band (4 waves each)
constexpr int H_ROWS = 4 * H_RG;
constexpr int H_CHUNK = 64;                     // source pixels staged at a time
constexpr int H_SEG_DW = (3 * H_CHUNK + 3 + 3) / 4;  // dwords that cover 3 * H_CHUNK bytes at any misalignment
// vertical pass: a workgroup makes 256 pixels (192 dwords) of one output row at a time
constexpr int V_PIX = 256;
constexpr int V_DW = 3 * V_PIX / 4;

struct PreTarget {
  int h, w;            // target size
  int kx, ky;          // row strides (ints) of the two coefficient tables
  int pitch;           // bytes of an intermediate row: 3 w rounded up to whole dwords
  long tab_off, tab_stride;      // the tables of image i begin at workspace + tab_off + i * tab_stride (bytes)
  long inter_off, inter_stride;  // the intermediate of image i
  float* out;          // [n_images, 3, h, w]
};

struct PreParams {
  const unsigned char* src;
  long long src_bytes;
  const long long* desc;  // device copy: {byte offset, H, W} per image
  int n_images, h_max, w_max, normalize;
  unsigned char* ws;
  PreTarget t[2];
};

// tables of one (image, target), ints: [x bounds 2 w][x coefficients w kx][y bounds 2 h][y coefficients h ky]
__host__ __device__ inline long table_ints(int h, int w, int kx, int ky) { return 2l * w + (long)w * kx + 2l * h + (long)h * ky; }

struct Image {
  long off;
  int H, W;
  bool ok;
};

// the device descriptor, checked against what the host planned from its own copy
__device__ __forceinline__ Image load_image(const PreParams& P, int i) {
  const long long* d = P.desc + 3l * i;
  const long long off = d[0], H = d[1], W = d[2];
  Image m;
  m.ok = off >= 0 && H >= 1 && H <= P.h_max && W >= 1 && W <= P.w_max && off + 3 * H * W <= P.src_bytes;
  m.off = (long)off, m.H = (int)H, m.W = (int)W;
  return m;
}

__device__ __forceinline__ double bicubic(double x) {
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// grid (blocks, image, 2 targets + 1): z = 2 t + axis (0: x, 1: y); the last z slice of image 0 builds the normalisation table
__global__ __launch_bounds__(PRE_THREADS) void preprocess_coeff_kernel(const PreParams P, int n_targets) {
  const int z = blockIdx.z;
  const int idx = blockIdx.x * PRE_THREADS + threadIdx.x;
  if (z == 2 * n_targets) {
    if (blockIdx.y != 0 || idx >= 768) return;
    // (float32(u) / float32(255) - mean_c) / std_c in float32.  The quotient of two float32 values formed in float64 and rounded
    // once more is the correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits), whatever the float32 division instruction does.
    const int c = idx >> 8, u = idx & 255;
    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
    const float std_ = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    float v = (float)((double)(float)u / 255.0);
    if (P.normalize) {
      const float d = v - mean;
      v = (float)((double)d / (double)std_);
    }
    reinterpret_cast<float*>(P.ws)[idx] = v;
    return;
  }
  const PreTarget T = (z >> 1) ? P.t[1] : P.t[0];
  const int axis = z & 1;
  const Image im = load_image(P, blockIdx.y);
  if (!im.ok) return;
  const int n_in = axis ? im.H : im.W, n_out = axis ? T.h : T.w;
  if (n_in == n_out || idx >= n_out) return;  // an axis that keeps its size has no pass and no table
  int* tab = reinterpret_cast<int*>(P.ws + T.tab_off + (long)blockIdx.y * T.tab_stride);
  int* bounds = axis ? tab + 2l * T.w + (long)T.w * T.kx : tab;
  int* K = bounds + 2l * n_out;
  const int kstride = axis ? T.ky : T.kx;

  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  const double ss = 1.0 / fs;
  const double center = ((double)idx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > n_in) xmax = n_in;
  int n = xmax - xmin;
  n = n < 0 ? 0 : (n > kstride ? kstride : n);  // never binds: n <= min(2 ceil(support), n_in) <= the stride (preprocess_plan)
  double ww = 0.0;
  for (int i = 0; i < n; ++i) ww += bicubic(((double)(i + xmin) - center + 0.5) * ss);
  int* row = K + (long)idx * kstride;
  for (int i = 0; i < n; ++i) {
    double k = bicubic(((double)(i + xmin) - center + 0.5) * ss);
    if (ww != 0.0) k /= ww;
    row[i] = k < 0.0 ? (int)(k * (double)(1 << PRECISION_BITS) - 0.5) : (int)(k * (double)(1 << PRECISION_BITS) + 0.5);
  }
  bounds[2 * idx] = xmin;
  bounds[2 * idx + 1] = n;
}

// dword at byte `idx` (a multiple of 4) of a 4-byte aligned array of `limit` bytes; bytes at or beyond the limit are never read
__device__ __forceinline__ unsigned load_dword_guarded(const unsigned char* base, long idx, long limit) {
  if (idx + 4 <= limit) return *reinterpret_cast<const unsigned*>(base + idx);
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (idx + k < limit) v |= (unsigned)base[idx + k] << (8 * k);
  return v;
}

// the four bytes at any byte index, from aligned dword loads
__device__ __forceinline__ unsigned load_4_bytes(const unsigned char* base, long idx, long limit) {
  const long a = idx & ~3l;
  const int sh = (int)(idx & 3) * 8;
  const unsigned lo = load_dword_guarded(base, a, limit);
  if (sh == 0) return lo;
  const unsigned hi = a + 4 < limit ? load_dword_guarded(base, a + 4, limit) : 0u;
  return (lo >> sh) | (hi << (32 - sh));
}

__device__ __forceinline__ unsigned clip8(int acc) {
  const int v = (acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS;  // arithmetic shift
  int c = v < 0 ? 0 : (v > 255 ? 255 : v);
  // Opaque to the optimiser on purpose.  Left visible, two shift-and-clamp results that are then packed into one dword were
  // selected as one v_ashr_pk_u8_i32, and hipcc ORs the other two bytes into its result as if bits 31:16 of it were zero; on the
  // MI355X they were not: bytes 2 and 3 of every dword of the vertical pass came out wrong while bytes 0 and 1 were right.
  asm volatile("" : "+v"(c));
  return (unsigned)c;
}

// grid (blocks, image, target).  Work item = (band of 16 rows, strip of 256 output bytes); a thread owns one output dword of four
// rows (one per row group).  The source pixels a strip needs are staged 64 at a time - the tap count depends on the data (1031 -> 42
// has 99) - as aligned dwords (rows are 3 W bytes at any alignment), together with the coefficients that fall on them.
__global__ __launch_bounds__(PRE_THREADS) void preprocess_horizontal_kernel(const PreParams P) {
  __shared__ int s_xmin[H_STRIP_COLS + 1], s_n[H_STRIP_COLS + 1];
  __shared__ int s_k[H_STRIP_COLS * H_CHUNK];
  __shared__ unsigned s_seg[H_ROWS * H_SEG_DW];
  const PreTarget T = blockIdx.z ? P.t[1] : P.t[0];
  const Image im = load_image(P, blockIdx.y);
  if (!im.ok || im.W == T.w) return;
  const int* bounds = reinterpret_cast<const int*>(P.ws + T.tab_off + (long)blockIdx.y * T.tab_stride);
  const int* K = bounds + 2l * T.w;
  unsigned char* inter = P.ws + T.inter_off + (long)blockIdx.y * T.inter_stride;
  const int strips = (T.pitch + H_STRIP_BYTES - 1) / H_STRIP_BYTES, bands = (im.H + H_ROWS - 1) / H_ROWS;
  const int kc = T.kx < H_CHUNK ? T.kx : H_CHUNK;  // coefficients of one column that can fall on one chunk
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long row_bytes = 3l * im.W;

  for (long item = blockIdx.x; item < (long)strips * bands; item += gridDim.x) {
    const int band = (int)(item / strips), strip = (int)(item - (long)band * strips);
    const int b0 = strip * H_STRIP_BYTES;  // first output byte of the strip
    const int xs0 = b0 / 3;
    const int xs1 = std::min(T.w - 1, (b0 + H_STRIP_BYTES - 1) / 3);
    const int ncols = xs1 - xs0 + 1;
    __syncthreads();  // the previous item has been read
    for (int c = tid; c < ncols; c += PRE_THREADS) {
      s_xmin[c] = bounds[2 * (xs0 + c)];
      s_n[c] = std::min(bounds[2 * (xs0 + c) + 1], T.kx);
    }
    __syncthreads();
    // windows move right with x: the strip needs source pixels [c_begin, c_end)
    const int c_begin = s_xmin[0], c_end = std::min(im.W, s_xmin[ncols - 1] + s_n[ncols - 1]);
    // this thread's four output bytes: column within the strip (-1: padding of the row) and channel
    const int j0 = b0 + 4 * lane;
    int xl[4], ch[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = (j0 + k) / 3;
      ch[k] = (j0 + k) - 3 * x;
      xl[k] = x < T.w ? x - xs0 : -1;
    }
    int acc[H_RG][4];
#pragma unroll
    for (int g = 0; g < H_RG; ++g)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[g][k] = 0;

    for (int c0 = c_begin; c0 < c_end; c0 += H_CHUNK) {
      if (c0 != c_begin) __syncthreads();  // the previous chunk has been read
      // column c's coefficients for source pixels [c0, c0 + H_CHUNK): taps ia .. ia + kc, zero where the window has ended
      for (int e = tid; e < ncols * kc; e += PRE_THREADS) {
        const int c = e / kc, k = e - c * kc;
        const int xm = s_xmin[c];
        const int i = std::max(0, c0 - xm) + k;
        s_k[e] = (i < s_n[c] && xm + i < c0 + H_CHUNK) ? K[(long)(xs0 + c) * T.kx + i] : 0;
      }
      // source pixels [c0, c0 + len) of the band's rows, as the aligned dwords that hold them
      const int len = std::min(H_CHUNK, c_end - c0);
      for (int e = tid; e < H_ROWS * H_SEG_DW; e += PRE_THREADS) {
        const int r = e / H_SEG_DW, d = e - r * H_SEG_DW;
        const int y = band * H_ROWS + r;
        if (y < im.H) {
          const long g = im.off + (long)y * row_bytes + 3l * c0;
          const long ga = g & ~3l;
          if (ga + 4l * d < g + 3l * len) s_seg[e] = load_dword_guarded(P.src, ga + 4l * d, (long)P.src_bytes);
        }
      }
      __syncthreads();
#pragma unroll
      for (int g = 0; g < H_RG; ++g) {
        const int r = g * 4 + wave;
        const int y = band * H_ROWS + r;
        if (y >= im.H) continue;  // wave-uniform
        const int shift = (int)((im.off + (long)y * row_bytes + 3l * c0) & 3);
        const unsigned char* seg = reinterpret_cast<const unsigned char*>(&s_seg[r * H_SEG_DW]) + shift;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (xl[k] < 0) continue;
          const int xm = s_xmin[xl[k]];
          const int ia = std::max(0, c0 - xm), ib = std::min(s_n[xl[k]], c0 + H_CHUNK - xm);
          const int* kr = &s_k[xl[k] * kc];                            // tap ia + t
          const unsigned char* sp = seg + 3 * (xm + ia - c0) + ch[k];  // its source byte
          int a = acc[g][k];
          for (int t = 0; t < ib - ia; ++t) a += (int)sp[3 * t] * kr[t];
          acc[g][k] = a;
        }
      }
    }
    if (j0 < T.pitch) {
#pragma unroll
      for (int g = 0; g < H_RG; ++g) {
        const int y = band * H_ROWS + g * 4 + wave;
        if (y >= im.H) continue;
        // the padding bytes of a row have no taps: they are stored as 0
        *reinterpret_cast<unsigned*>(inter + (long)y * T.pitch + j0) =
            clip8(acc[g][0]) | (clip8(acc[g][1]) << 8) | (clip8(acc[g][2]) << 16) | (clip8(acc[g][3]) << 24);
      }
    }
  }
}

// grid (blocks, image, target).  Work item = (output row, segment of 256 pixels).  Threads 0 .. 191 walk down the columns of one
// dword (four bytes of the interleaved row) each, with wave-uniform coefficients; the four clamped bytes go through LDS to the
// thread of their pixel, which looks the three channels up in the normalisation table and stores one float into each plane.
__global__ __launch_bounds__(PRE_THREADS) void preprocess_vertical_kernel(const PreParams P) {
  __shared__ float s_norm[768];
  __shared__ unsigned s_row[V_DW];
  const PreTarget T = blockIdx.z ? P.t[1] : P.t[0];
  const Image im = load_image(P, blockIdx.y);
  if (!im.ok) return;
  const int tid = threadIdx.x;
  for (int e = tid; e < 768; e += PRE_THREADS) s_norm[e] = reinterpret_cast<const float*>(P.ws)[e];
  const bool hskip = im.W == T.w, vskip = im.H == T.h;
  // rows come from the intermediate, or straight from the source where the horizontal pass is skipped
  const unsigned char* in = hskip ? P.src : P.ws + T.inter_off + (long)blockIdx.y * T.inter_stride;
  const long in_off = hskip ? im.off : 0l, in_stride = hskip ? 3l * im.W : (long)T.pitch;
  const long in_limit = hskip ? (long)P.src_bytes : (long)im.H * T.pitch;
  const int* tab = reinterpret_cast<const int*>(P.ws + T.tab_off + (long)blockIdx.y * T.tab_stride);
  const int* yb = tab + 2l * T.w + (long)T.w * T.kx;
  const int* yK = yb + 2l * T.h;
  const int segs = (T.w + V_PIX - 1) / V_PIX;
  const long plane = (long)T.h * T.w;
  float* out = T.out + (long)blockIdx.y * 3 * plane;

  for (long item = blockIdx.x; item < (long)T.h * segs; item += gridDim.x) {
    const int y = (int)(item / segs), sg = (int)(item - (long)y * segs);
    const int ymin = vskip ? y : yb[2 * y];
    const int n = vskip ? 1 : std::min(yb[2 * y + 1], T.ky);
    const int* kr = yK + (long)y * T.ky;
    const long q = (long)sg * V_DW + tid;  // dword of the row
    __syncthreads();                       // the previous item has been read (first item: the table is in place)
    if (tid < V_DW && 4 * q < 3l * T.w) {
      int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      for (int i = 0; i < n; ++i) {
        const int k = vskip ? (1 << PRECISION_BITS) : kr[i];
        const unsigned v = load_4_bytes(in, in_off + (long)(ymin + i) * in_stride + 4 * q, in_limit);
        a0 += (int)(v & 255u) * k, a1 += (int)((v >> 8) & 255u) * k, a2 += (int)((v >> 16) & 255u) * k, a3 += (int)(v >> 24) * k;
      }
      s_row[tid] = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
    }
    __syncthreads();
    const int x = sg * V_PIX + tid;
    if (x < T.w) {
      const unsigned char* b = reinterpret_cast<const unsigned char*>(s_row) + 3 * tid;
      float* o = out + (long)y * T.w + x;
      o[0] = s_norm[b[0]];
      o[plane] = s_norm[256 + b[1]];
      o[2 * plane] = s_norm[512 + b[2]];
    }
  }
}

// Pillow's bound on the taps of one output coordinate; monotone in n_in
int ksize(int n_in, int n_out) {
  const double scale = (double)n_in / (double)n_out;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;
}

long round16(long v) { return (v + 15) & ~15l; }

struct Plan {
  PreTarget t[2];
  int h_max, w_max;
  bool any_horizontal;
  long bytes;
};

// every check of the descriptors and targets, and the workspace layout; src_bytes < 0: sizes only
int preprocess_plan(const long long* desc, int n_images, const int* targets_hw, int n_targets, long long src_bytes, Plan* plan) {
  ROMA_REQUIRE(desc && targets_hw, "preprocess: null pointer (descriptors or targets)");
  ROMA_REQUIRE(n_targets == 1 || n_targets == 2, "preprocess: n_targets must be 1 or 2");
  ROMA_REQUIRE(n_images >= 1 && n_images <= 65535, "preprocess: n_images must lie in [1, 65535]");
  for (int k = 0; k < n_targets; ++k)
    ROMA_REQUIRE(targets_hw[2 * k] >= 1 && targets_hw[2 * k + 1] >= 1 && targets_hw[2 * k] <= MAX_SIDE && targets_hw[2 * k + 1] <= MAX_SIDE,
                 "preprocess: a target size is below 1 or above 32768");
  int h_max = 0, w_max = 0;
  for (int i = 0; i < n_images; ++i) {
    const long long off = desc[3 * i], H = desc[3 * i + 1], W = desc[3 * i + 2];
    ROMA_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE,
                 "preprocess: image " + std::to_string(i) + " has a size (H or W) below 1 or above 32768");
    ROMA_REQUIRE(off >= 0, "preprocess: image " + std::to_string(i) + " has a negative offset");
    ROMA_REQUIRE(src_bytes < 0 || (off <= src_bytes && 3 * H * W <= src_bytes - off),
                 "preprocess: image " + std::to_string(i) + " ends beyond src_bytes (offset + 3 H W > src_bytes)");
    h_max = std::max(h_max, (int)H), w_max = std::max(w_max, (int)W);
  }
  plan->h_max = h_max, plan->w_max = w_max, plan->any_horizontal = false;
  long at = NORM_BYTES;
  for (int k = 0; k < n_targets; ++k) {
    PreTarget& T = plan->t[k];
    T.h = targets_hw[2 * k], T.w = targets_hw[2 * k + 1];
    T.kx = std::min(ksize(w_max, T.w), w_max), T.ky = std::min(ksize(h_max, T.h), h_max);
    T.pitch = (3 * T.w + 3) & ~3;
    T.tab_stride = round16(table_ints(T.h, T.w, T.kx, T.ky) * (long)sizeof(int));
    T.tab_off = at;
    at += T.tab_stride * n_images;
    T.out = nullptr;
    for (int i = 0; i < n_images; ++i) plan->any_horizontal = plan->any_horizontal || desc[3 * i + 2] != T.w;
  }
  for (int k = 0; k < n_targets; ++k) {
    PreTarget& T = plan->t[k];
    T.inter_stride = round16((long)h_max * T.pitch);
    T.inter_off = at;
    at += T.inter_stride * n_images;
  }
  if (n_targets == 1) plan->t[1] = plan->t[0];
  plan->bytes = at;
  return 0;
}

unsigned grid_x(long items, int slices) {
  return (unsigned)std::max<long>(1, std::min<long>(items, std::max(1, PRE_MAX_BLOCKS / slices)));
}

}  // namespace

extern "C" long roma_op_preprocess_workspace(const long long* desc_host, int n_images, const int* targets_hw, int n_targets) {
  Plan plan;
  if (preprocess_plan(desc_host, n_images, targets_hw, n_targets, -1, &plan) != 0) return -1;
  return plan.bytes;
}

extern "C" int roma_op_preprocess(const unsigned char* src, long long src_bytes, const long long* desc_host, const long long* desc_dev,
                                  int n_images, const int* targets_hw, int n_targets, int normalize, float* out0, float* out1,
                                  void* workspace, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(src && desc_host && desc_dev && targets_hw && out0 && workspace, "preprocess: null pointer");
  ROMA_REQUIRE(n_targets != 2 || out1, "preprocess: null pointer (out1 with two targets)");
  ROMA_REQUIRE(src_bytes >= 0, "preprocess: src_bytes is negative");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(desc_dev) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "preprocess: src must be 4-byte, desc_dev 8-byte and workspace 16-byte aligned");
  Plan plan;
  if (preprocess_plan(desc_host, n_images, targets_hw, n_targets, src_bytes, &plan) != 0) return -1;
  plan.t[0].out = out0;
  plan.t[1].out = n_targets == 2 ? out1 : out0;
  PreParams P = {src, src_bytes, desc_dev, n_images, plan.h_max, plan.w_max, normalize ? 1 : 0, static_cast<unsigned char*>(workspace),
                 {plan.t[0], plan.t[1]}};
  const int slices = n_images * n_targets;
  long coeff_items = 768, h_items = 0, v_items = 0;
  for (int k = 0; k < n_targets; ++k) {
    const PreTarget& T = plan.t[k];
    coeff_items = std::max<long>(coeff_items, std::max(T.h, T.w));
    h_items = std::max(h_items, (long)((T.pitch + H_STRIP_BYTES - 1) / H_STRIP_BYTES) * ((plan.h_max + H_ROWS - 1) / H_ROWS));
    v_items = std::max(v_items, (long)T.h * ((T.w + V_PIX - 1) / V_PIX));
  }
  // algorithmic bytes of the two passes, with every image counted at the size of the largest: source in and intermediate out;
  // intermediate in and three float planes out
  double h_bytes = 0.0, v_bytes = 0.0;
  for (int k = 0; k < n_targets; ++k) {
    const double inter = (double)n_images * plan.h_max * plan.t[k].pitch;
    h_bytes += (double)src_bytes + inter;
    v_bytes += inter + (double)n_images * 12.0 * plan.t[k].h * plan.t[k].w;
  }
  {
    ProfScope ps("preprocess_coeff_kernel", (double)slices * 2.0 * (double)coeff_items * 64.0, "B", s);
    hipLaunchKernelGGL(preprocess_coeff_kernel, dim3((unsigned)((coeff_items + PRE_THREADS - 1) / PRE_THREADS), n_images, 2 * n_targets + 1),
                       dim3(PRE_THREADS), 0, s, P, n_targets);
    ROMA_LAUNCH_CHECK();
  }
  if (plan.any_horizontal) {
    ProfScope ps("preprocess_horizontal_kernel", h_bytes, "B", s);
    hipLaunchKernelGGL(preprocess_horizontal_kernel, dim3(grid_x(h_items, slices), n_images, n_targets), dim3(PRE_THREADS), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  {
    ProfScope ps("preprocess_vertical_kernel", v_bytes, "B", s);
    hipLaunchKernelGGL(preprocess_vertical_kernel, dim3(grid_x(v_items, slices), n_images, n_targets), dim3(PRE_THREADS), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace roma
