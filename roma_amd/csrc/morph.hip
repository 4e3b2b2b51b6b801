// Warp morph rendering (roma_op_render_morph): the T frames  grid_sample(image, (1 - t) warp[..., :2] + t warp[..., 2:])  of the
// reference's demo/demo_3D_effect.py, optionally blended over a background by the certainty as visualize_warp does, written as
// uint8 [B, T, H, W, 3] (what tensor_to_pil makes of a frame) or f32 [B, T, 3, H, W].  The definition is stated in
// include/roma_hip.h and restated, operation by operation, in numpy float32 by tools/morph_ref.py - the oracle of
// tests/test_gpu_morph.py.
//
// Two kernels on the caller's stream, nothing read back, nothing allocated:
//   1. morph_pack_kernel    the image (f32 planar, or uint8 interleaved as float(u) / 255.f) into interleaved 16-byte texels
//                           (r, g, b, 0) in the caller's workspace, one all-zero texel in front of every image, and the T pairs of
//                           frame weights (float(1 - t), float(t)), formed in float64 and rounded once;
//   2. render_morph_kernel  a wave renders 256 consecutive pixels of the flattened H x W frame, four per lane (lane l the pixels l,
//                           64 + l, 128 + l, 192 + l, so the lanes of every load and store are neighbouring pixels): their warp
//                           rows (and certainty) are loaded once, then a loop over a chunk of MORPH_FRAME_CHUNK frames forms the
//                           coordinates, fetches the four taps of a pixel as four 16-byte loads and writes the wave's 768 bytes of
//                           the frame - through the wave's slice of LDS, out as three coalesced dwords per lane.  Frame chunks
//                           and the batch are the other two grid axes.
// A tap out of range reads the zero texel instead of being skipped: weight * 0 = +0 and x + 0 = x, so the sum has the bits of the
// sum that skips it, and no texel that the tap does not cover (a NaN in the picture, say) can reach the pixel.
// A frame whose first byte is not dword aligned (H W 3 is odd, say) and the last, partial wave of a frame are written byte by
// byte from registers; the f32 form stores one coalesced dword per lane, pixel and channel.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/roma_hip.h"
#include "common.h"

// nothing here is fused: tools/morph_ref.py evaluates the same float32 expressions in the same order
#pragma clang fp contract(off)

namespace roma {
namespace {

constexpr int MORPH_THREADS = 256;
constexpr int MORPH_WAVES = MORPH_THREADS / 64;
constexpr int MORPH_GROUP = 4;  // pixels per thread
constexpr int MORPH_WAVE_PIXELS = 64 * MORPH_GROUP;  // 768 bytes of a uint8 frame: three dwords per lane
constexpr int MORPH_FRAME_CHUNK = 32;  // frames per workgroup: the warp is re-read (from cache) once per chunk
constexpr int MORPH_XCDS = 8;  // dies with an L2 of their own
constexpr int MORPH_MAX_SIDE = 32768;
constexpr long MORPH_MAX_FRAMES = 65535l * MORPH_FRAME_CHUNK;

struct PackParams {
  const void* image;
  int image_u8;
  const double* ts;
  int B, h, w;
  long T;
  f32x4* texels;   // [B, 1 + h w]
  float* weights;  // [T, 2]
};

// one thread per texel of [B, 1 + h w], then one per frame
__global__ __launch_bounds__(MORPH_THREADS) void morph_pack_kernel(const PackParams A) {
  const long hw = (long)A.h * A.w, per = hw + 1, n_tex = (long)A.B * per;
  const long i = (long)blockIdx.x * MORPH_THREADS + threadIdx.x;
  if (i < n_tex) {
    const long b = i / per, k = i - b * per;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k > 0) {
      if (A.image_u8) {
        const unsigned char* p = static_cast<const unsigned char*>(A.image) + (b * hw + (k - 1)) * 3;
        v[0] = (float)p[0] / 255.f, v[1] = (float)p[1] / 255.f, v[2] = (float)p[2] / 255.f;
      } else {
        const float* p = static_cast<const float*>(A.image) + b * 3 * hw + (k - 1);
        v[0] = p[0], v[1] = p[hw], v[2] = p[2 * hw];
      }
    }
    A.texels[i] = v;
  } else if (i < n_tex + A.T) {
    const long t = i - n_tex;
    const double tt = A.ts[t];
    A.weights[2 * t] = (float)(1.0 - tt), A.weights[2 * t + 1] = (float)tt;
  }
}

struct MorphParams {
  const float* warp;
  long warp_bs, warp_rs;  // floats
  const float* cert;
  long cert_bs, cert_rs;  // floats
  float background;
  const f32x4* texels;
  const float* weights;
  long T;
  int H, W, h, w;
  void* out;
};

// x or y of the interpolated warp to a pixel coordinate of the image, as visualize_warp_kernel does it
__device__ __forceinline__ float unnormalise(float g, float size) {
  const float i = ((g + 1.f) * size - 1.f) * 0.5f;
  return fminf(fmaxf(i, -1.0e6f), 1.0e6f);
}

// bilinear, zeros padding, of the texels of one image (tex[0] is the zero texel) at pixel coordinates (ix, iy)
__device__ __forceinline__ void sample3(const f32x4* tex, int h, int w, float ix, float iy, float* rgb) {
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float tx = ix - fx0, ty = iy - fy0;
  const float ux = 1.f - tx, uy = 1.f - ty;
  const float wgt[4] = {ux * uy, tx * uy, ux * ty, tx * ty};
  const bool w_in = (unsigned)x0 < (unsigned)w, e_in = (unsigned)(x0 + 1) < (unsigned)w;
  const bool n_in = (unsigned)y0 < (unsigned)h, s_in = (unsigned)(y0 + 1) < (unsigned)h;
  // |y0| <= 1e6 times w <= 32768 does not fit 32 bits: unsigned arithmetic wraps, and an index is used only where its tap is in
  // range, where it is 1 + y w + x <= h w <= 2^30
  const unsigned row_n = (unsigned)y0 * (unsigned)w + (unsigned)x0 + 1u, row_s = row_n + (unsigned)w;
  const unsigned idx[4] = {(n_in && w_in) ? row_n : 0u, (n_in && e_in) ? row_n + 1u : 0u, (s_in && w_in) ? row_s : 0u,
                           (s_in && e_in) ? row_s + 1u : 0u};
  f32x4 v[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = tex[idx[t]];
  rgb[0] = rgb[1] = rgb[2] = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] + wgt[t] * v[t][c];
  }
}

// truncation after the clip, as numpy_to_pil does it; NaN -> 0
__device__ __forceinline__ unsigned to_u8(float v) { return (unsigned)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

// what one lane of a wave wrote to LDS, every lane of that wave may read after this (and the other way round): a wave's LDS
// operations execute in order, so ordering the compiler's accesses is all that is needed - no s_barrier, and waves that have
// left the kernel (past the end of the frame) are not waited for
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// grid (H W / 1024, frame chunks, B), its first two axes remapped below: a wave renders 256 consecutive pixels of the flattened frame, lane l the pixels l, 64 + l,
// 128 + l, 192 + l of them, so that the lanes of one load or store are neighbouring pixels
template <bool OUT_U8, bool CERT>
__global__ __launch_bounds__(MORPH_THREADS) void render_morph_kernel(const MorphParams A) {
  __shared__ uint32_t s_stage[MORPH_WAVES][MORPH_WAVE_PIXELS * 3 / 4];
  const int b = blockIdx.z;
  const int n = A.H * A.W;  // <= 2^30
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // Which (pixel block, frame chunk) this workgroup renders.  Workgroups are dealt to the 8 XCDs in turn, and each XCD has its own
  // L2: the workgroups with the same dispatch index modulo 8 take a contiguous band of pixel blocks, all frame chunks of a block
  // one after the other, so that an XCD gathers from the band of the picture its pixels point into and not from all of it.  A
  // bijection of the (x, y) grid for every size; it moves work between workgroups, no bit of the output depends on it.
  const unsigned long nx = gridDim.x, ny = gridDim.y, total = nx * ny, lin = blockIdx.x + nx * blockIdx.y;
  const unsigned long grp = lin % MORPH_XCDS, logical = grp * (total / MORPH_XCDS) + min(grp, total % MORPH_XCDS) + lin / MORPH_XCDS;
  const unsigned long block = logical / ny, chunk = logical - block * ny;
  const long first = ((long)block * MORPH_WAVES + wave) * MORPH_WAVE_PIXELS;
  if (first >= n) return;  // the whole wave
  const int p0 = (int)first;
  const bool full = n - p0 >= MORPH_WAVE_PIXELS;
  float ax[MORPH_GROUP], ay[MORPH_GROUP], bx[MORPH_GROUP], by[MORPH_GROUP], ce[MORPH_GROUP], bg[MORPH_GROUP];
  const float* warp = A.warp + (long)b * A.warp_bs;
#pragma unroll
  for (int j = 0; j < MORPH_GROUP; ++j) {
    const int p = min(p0 + 64 * j + lane, n - 1);  // a pixel past the end repeats the last one and is not stored
    const int row = p / A.W, col = p - row * A.W;
    const f32x4 m = *reinterpret_cast<const f32x4*>(warp + (long)row * A.warp_rs + 4l * col);
    ax[j] = m[0], ay[j] = m[1], bx[j] = m[2], by[j] = m[3];
    if (CERT) {
      ce[j] = A.cert[(long)b * A.cert_bs + (long)row * A.cert_rs + col];
      bg[j] = (1.f - ce[j]) * A.background;
    }
  }
  const f32x4* tex = A.texels + (long)b * ((long)A.h * A.w + 1);
  const float wf = (float)A.w, hf = (float)A.h;
  const long t0 = (long)chunk * MORPH_FRAME_CHUNK, t1 = std::min<long>(A.T, t0 + MORPH_FRAME_CHUNK);
  for (long t = t0; t < t1; ++t) {
    const float w0 = A.weights[2 * t], w1 = A.weights[2 * t + 1];
    float v[MORPH_GROUP][3];
#pragma unroll
    for (int j = 0; j < MORPH_GROUP; ++j) {
      const float gx = w0 * ax[j] + w1 * bx[j], gy = w0 * ay[j] + w1 * by[j];
      sample3(tex, A.h, A.w, unnormalise(gx, wf), unnormalise(gy, hf), v[j]);
      if (CERT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = ce[j] * v[j][c] + bg[j];
      }
    }
    const long frame = (long)b * A.T + t;
    if (OUT_U8) {
      unsigned char* o = static_cast<unsigned char*>(A.out) + (frame * n + p0) * 3;  // the wave's 768 bytes of this frame
      if (full && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        // bytes through the wave's LDS slice, out as three coalesced dwords per lane
        unsigned char* st = reinterpret_cast<unsigned char*>(s_stage[wave]);
#pragma unroll
        for (int j = 0; j < MORPH_GROUP; ++j) {
#pragma unroll
          for (int c = 0; c < 3; ++c) st[(64 * j + lane) * 3 + c] = (unsigned char)to_u8(v[j][c]);
        }
        wave_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<uint32_t*>(o)[64 * k + lane] = s_stage[wave][64 * k + lane];
        wave_sync();
      } else {
#pragma unroll
        for (int j = 0; j < MORPH_GROUP; ++j) {
          if (p0 + 64 * j + lane < n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(64 * j + lane) * 3 + c] = (unsigned char)to_u8(v[j][c]);
          }
        }
      }
    } else {
      float* o = static_cast<float*>(A.out) + frame * 3 * n + p0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int j = 0; j < MORPH_GROUP; ++j) {
          if (p0 + 64 * j + lane < n) o[(long)c * n + 64 * j + lane] = v[j][c];
        }
      }
    }
  }
}

bool side_ok(int v) { return v >= 1 && v <= MORPH_MAX_SIDE; }

long texel_bytes(int B, int h, int w) { return (long)B * ((long)h * w + 1) * 16; }

// [p, p + bytes) and [q, q + bytes_q) share a byte
bool overlap(const void* p, long bytes, const void* q, long bytes_q) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q);
  return a < c + (uintptr_t)bytes_q && c < a + (uintptr_t)bytes;
}

}  // namespace

extern "C" int roma_op_render_morph_frame_chunk(void) { return MORPH_FRAME_CHUNK; }

extern "C" long roma_op_render_morph_workspace(int B, int im_h, int im_w, long T) {
  if (B < 1 || B > 65535 || !side_ok(im_h) || !side_ok(im_w) || T < 1 || T > MORPH_MAX_FRAMES) return -1;
  return texel_bytes(B, im_h, im_w) + T * 8;
}

extern "C" int roma_op_render_morph(const float* warp, long warp_bs, long warp_rs, const void* image, int image_u8, const double* ts,
                                    const float* certainty, long cert_bs, long cert_rs, float background, int B, long T, int H, int W,
                                    int im_h, int im_w, void* out, int out_f32, void* workspace, long workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  ROMA_REQUIRE(warp && image && ts && out && workspace, "render_morph: null pointer");
  ROMA_REQUIRE(B >= 1 && B <= 65535, "render_morph: B must lie in [1, 65535]");
  ROMA_REQUIRE(T >= 1 && T <= MORPH_MAX_FRAMES, "render_morph: T (frames) must lie in [1, 65535 * 32]");
  ROMA_REQUIRE(side_ok(H) && side_ok(W), "render_morph: the warp grid (H, W) must lie in [1, 32768]^2");
  ROMA_REQUIRE(side_ok(im_h) && side_ok(im_w), "render_morph: the image size (h, w) must lie in [1, 32768]^2");
  ROMA_REQUIRE(image_u8 == 0 || image_u8 == 1, "render_morph: image_u8 must be 0 (float32 [B, 3, h, w]) or 1 (uint8 [B, h, w, 3])");
  ROMA_REQUIRE(out_f32 == 0 || out_f32 == 1, "render_morph: out_f32 must be 0 (uint8 [B, T, H, W, 3]) or 1 (float32 [B, T, 3, H, W])");
  const long n = (long)H * W;
  ROMA_REQUIRE((double)B * (double)T * (double)n * 3.0 < 9.0e15, "render_morph: B * T * H * W * 3 is beyond what the output index holds");
  ROMA_REQUIRE(warp_rs >= 4l * W && warp_rs % 4 == 0 && warp_bs >= (long)(H - 1) * warp_rs + 4l * W && warp_bs % 4 == 0,
               "render_morph: warp strides (in floats) must be multiples of 4 with row_stride >= 4 W and batch_stride >= (H - 1) "
               "row_stride + 4 W");
  ROMA_REQUIRE(!certainty || (cert_rs >= W && cert_bs >= (long)(H - 1) * cert_rs + W),
               "render_morph: certainty strides (in floats) must have row_stride >= W and batch_stride >= (H - 1) row_stride + W");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(warp) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "render_morph: warp and workspace must be 16-byte aligned");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(ts) & 7) == 0 && (!certainty || (reinterpret_cast<uintptr_t>(certainty) & 3) == 0) &&
                   (image_u8 || (reinterpret_cast<uintptr_t>(image) & 3) == 0) && (!out_f32 || (reinterpret_cast<uintptr_t>(out) & 3) == 0),
               "render_morph: ts, certainty, a float32 image or a float32 out is not aligned to its type");
  ROMA_REQUIRE(background == background, "render_morph: background is NaN");
  const long need = roma_op_render_morph_workspace(B, im_h, im_w, T);
  ROMA_REQUIRE(workspace_bytes >= need, "render_morph: workspace is too small");
  // what is written must not share a byte with what is read, nor the two written buffers with each other
  const long out_bytes = (long)B * T * n * 3 * (out_f32 ? 4 : 1);
  const long warp_bytes = ((long)(B - 1) * warp_bs + (long)(H - 1) * warp_rs + 4l * W) * 4;
  const long image_bytes = (long)B * 3 * im_h * im_w * (image_u8 ? 1 : 4);
  const long cert_bytes = certainty ? ((long)(B - 1) * cert_bs + (long)(H - 1) * cert_rs + W) * 4 : 0;
  for (int k = 0; k < 2; ++k) {
    const void* dst = k ? workspace : out;
    const long dst_bytes = k ? need : out_bytes;
    ROMA_REQUIRE(!overlap(dst, dst_bytes, warp, warp_bytes) && !overlap(dst, dst_bytes, image, image_bytes) &&
                     !overlap(dst, dst_bytes, ts, T * 8) && !(certainty && overlap(dst, dst_bytes, certainty, cert_bytes)),
                 "render_morph: out or workspace aliases an input");
  }
  ROMA_REQUIRE(!overlap(out, out_bytes, workspace, need), "render_morph: out aliases workspace");

  f32x4* texels = static_cast<f32x4*>(workspace);
  float* weights = reinterpret_cast<float*>(static_cast<char*>(workspace) + texel_bytes(B, im_h, im_w));
  {
    PackParams P = {image, image_u8, ts, B, im_h, im_w, T, texels, weights};
    const long threads = (long)B * ((long)im_h * im_w + 1) + T;
    ProfScope ps("morph_pack_kernel", (double)threads * 28.0, "B", s);
    hipLaunchKernelGGL(morph_pack_kernel, dim3((unsigned)((threads + MORPH_THREADS - 1) / MORPH_THREADS)), dim3(MORPH_THREADS), 0, s, P);
    ROMA_LAUNCH_CHECK();
  }
  MorphParams A = {warp, warp_bs, warp_rs, certainty, cert_bs, cert_rs, background, texels, weights, T, H, W, im_h, im_w, out};
  const long block_pixels = (long)MORPH_WAVES * MORPH_WAVE_PIXELS;
  const dim3 grid((unsigned)((n + block_pixels - 1) / block_pixels), (unsigned)((T + MORPH_FRAME_CHUNK - 1) / MORPH_FRAME_CHUNK), B);
  ProfScope ps("render_morph_kernel", (double)out_bytes, "B", s);
  if (out_f32) {
    if (certainty) hipLaunchKernelGGL((render_morph_kernel<false, true>), grid, dim3(MORPH_THREADS), 0, s, A);
    else hipLaunchKernelGGL((render_morph_kernel<false, false>), grid, dim3(MORPH_THREADS), 0, s, A);
  } else {
    if (certainty) hipLaunchKernelGGL((render_morph_kernel<true, true>), grid, dim3(MORPH_THREADS), 0, s, A);
    else hipLaunchKernelGGL((render_morph_kernel<true, false>), grid, dim3(MORPH_THREADS), 0, s, A);
  }
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
