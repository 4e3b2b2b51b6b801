// HBM-bound kernels of the RoMa match() path for gfx950 (see elementwise.h); the ConvRefiner's are refiner_input.hip,
// refiner_out.hip and dwconv5x5.hip.  Conventions: channels-last activations, 16-byte (or 8-byte for bf16 quads) vector
// accesses, one wave64 per row for row reductions, f32 math everywhere.
#include <algorithm>
#include "elementwise_device.h"
#include "chol_diag.h"

namespace roma {

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ------------------------------------------------------------------ LayerNorm
template <typename TIN, typename TOUT>
__global__ __launch_bounds__(256) void layernorm_kernel(const TIN* x, const float* w, const float* b, TOUT* out,
                                                        long M, int D, float eps) {
  // one wave per row; a lane owns 8 consecutive elements of every 512-element chunk (two 16-byte loads, one 16-byte
  // bf16 store): the previous 4-element mapping wrote 8-byte pieces and ran at 2.9 TB/s
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const TIN* xr = x + row * D;
  f32x4 v[4][2];
  const int nv = D / 512;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) {
      if constexpr (sizeof(TIN) == 2) {  // bf16 residual stream: one 16-byte load, widened exactly
        const uint4 r = *reinterpret_cast<const uint4*>(xr + i * 512 + lane * 8);
        const unsigned rp[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[i][j >> 1][2 * (j & 1)] = h16_lo(rp[j]);
          v[i][j >> 1][2 * (j & 1) + 1] = h16_hi(rp[j]);
        }
      } else {
        v[i][0] = *reinterpret_cast<const f32x4*>(xr + i * 512 + lane * 8);
        v[i][1] = *reinterpret_cast<const f32x4*>(xr + i * 512 + lane * 8 + 4);
      }
    }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) s += (v[i][0][0] + v[i][0][1] + v[i][0][2] + v[i][0][3]) + (v[i][1][0] + v[i][1][1] + v[i][1][2] + v[i][1][3]);
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = v[i][u][j] - mean;
          q += d * d;
        }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nv) {
      const int c = i * 512 + lane * 8;
      f32x4 o[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c + 4 * u);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b + c + 4 * u);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[u][j] = (v[i][u][j] - mean) * rstd * wv[j] + bv[j];
      }
      if constexpr (sizeof(TOUT) == 2) {
        uint4 pk;
        pk.x = pack_bf16x2(o[0][0], o[0][1]);
        pk.y = pack_bf16x2(o[0][2], o[0][3]);
        pk.z = pack_bf16x2(o[1][0], o[1][1]);
        pk.w = pack_bf16x2(o[1][2], o[1][3]);
        *reinterpret_cast<uint4*>(out + row * D + c) = pk;
      } else {
        ElemIO<TOUT>::st4(out + row * D + c, o[0]);
        ElemIO<TOUT>::st4(out + row * D + c + 4, o[1]);
      }
    }
}

int layernorm_launch_dt(const void* x, int dt_in, const float* w, const float* b, void* out, long M, int D, float eps,
                        int dt_out, hipStream_t s) {
  ROMA_REQUIRE(D % 512 == 0 && D <= 2048, "layernorm: D must be a multiple of 512 and <= 2048");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
               "layernorm: x / out not 16-byte aligned");
  dim3 grid((unsigned)((M + 3) / 4));
  if (dt_in == DT_BF16) {
    ROMA_REQUIRE(dt_out == DT_BF16, "layernorm: bf16 input implies bf16 output");
    hipLaunchKernelGGL((layernorm_kernel<bf16_t, bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)x, w, b, (bf16_t*)out, M, D, eps);
  } else {
    ROMA_DT_SWITCH(dt_out, T, hipLaunchKernelGGL((layernorm_kernel<float, T>), grid, dim3(256), 0, s, (const float*)x, w, b,
                                                 (T*)out, M, D, eps));
  }
  ROMA_LAUNCH_CHECK();
  return 0;
}

int layernorm_launch(const float* x, const float* w, const float* b, void* out, long M, int D, float eps,
                     int dt_out, hipStream_t s) {
  return layernorm_launch_dt(x, DT_F32, w, b, out, M, D, eps, dt_out, s);
}

// ------------------------------------------------------------------ conv3x3, Cin = 3 (first VGG layer)
template <typename TOUT>
__global__ __launch_bounds__(256) void conv3x3_c3_kernel(const float* img, const float* w, const float* bias,
                                                         TOUT* out, int B, int H, int W) {
  __shared__ __attribute__((aligned(16))) float ws[27 * 64];
  __shared__ float bs[64];
  for (int i = threadIdx.x; i < 27 * 64; i += 256) ws[i] = w[i];
  if (threadIdx.x < 64) bs[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const long HW = (long)H * W;
  const long pix = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int cg = threadIdx.x & 3;  // 16 output channels each
  if (pix >= (long)B * HW) return;
  const int b = (int)(pix / HW);
  const int rem = (int)(pix - (long)b * HW);
  const int y = rem / W, x = rem - y * W;
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = bs[cg * 16 + j];
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = img[((long)(b * 3 + ci) * H + yy) * W + xx];
        const float* wr = &ws[(ci * 9 + ky * 3 + kx) * 64 + cg * 16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = fmaf(v, wr[j], acc[j]);
      }
  TOUT* o = out + pix * 64 + cg * 16;
#pragma unroll
  for (int j4 = 0; j4 < 4; ++j4) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(acc[j4 * 4 + j], 0.f);
    ElemIO<TOUT>::st4(o + j4 * 4, v);
  }
}

int conv3x3_c3_launch(const float* img, const float* w, const float* bias, void* out, int B, int H, int W,
                      int dt_out, hipStream_t s) {
  const long total = (long)B * H * W;
  dim3 grid((unsigned)((total + 63) / 64));
  ROMA_DT_SWITCH(dt_out, T, hipLaunchKernelGGL(conv3x3_c3_kernel<T>, grid, dim3(256), 0, s, img, w, bias, (T*)out, B, H, W));
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ im2col for the first 3x3 layer (K = 27 -> 32)
template <typename TOUT>
__global__ __launch_bounds__(256) void im2col3x3_c3_kernel(const float* img, TOUT* out, int B, int H, int W) {
  const long HW = (long)H * W;
  const long total = (long)B * HW * 8;  // 8 quads of 4 taps per pixel
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int quad = (int)(idx & 7);
    const long pix = idx >> 3;
    const int b = (int)(pix / HW);
    const int rem = (int)(pix - (long)b * HW);
    const int y = rem / W, x = rem - y * W;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = quad * 4 + j;
      float val = 0.f;
      if (k < 27) {
        const int ci = k / 9, t = k - ci * 9, ky = t / 3, kx = t - ky * 3;
        const int yy = y + ky - 1, xx = x + kx - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) val = img[((long)(b * 3 + ci) * H + yy) * W + xx];
      }
      v[j] = val;
    }
    ElemIO<TOUT>::st4(out + pix * 32 + quad * 4, v);
  }
}

int im2col3x3_c3_launch(const float* img, void* out, int B, int H, int W, int dt_out, hipStream_t s) {
  const long total = (long)B * H * W * 8;
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1 << 20));
  ROMA_DT_SWITCH(dt_out, T, hipLaunchKernelGGL(im2col3x3_c3_kernel<T>, grid, dim3(256), 0, s, img, (T*)out, B, H, W));
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ MaxPool 2x2
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* in, T* out, int B, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const long total = (long)B * Ho * Wo * C4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C4) * 4;
    long r = idx / C4;
    const int xo = (int)(r % Wo);
    r /= Wo;
    const int yo = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const T* p = in + (((long)b * H + 2 * yo) * W + 2 * xo) * C + c;
    const f32x4 a0 = ElemIO<T>::ld4(p), a1 = ElemIO<T>::ld4(p + C), a2 = ElemIO<T>::ld4(p + (long)W * C),
                a3 = ElemIO<T>::ld4(p + (long)W * C + C);
    f32x4 m;
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = fmaxf(fmaxf(a0[j], a1[j]), fmaxf(a2[j], a3[j]));
    ElemIO<T>::st4(out + (((long)b * Ho + yo) * Wo + xo) * C + c, m);
  }
}

int maxpool2x2_launch(const void* in, void* out, int B, int H, int W, int C, int dt, hipStream_t s) {
  ROMA_REQUIRE(C % 4 == 0, "maxpool: C must be a multiple of 4");
  const long total = (long)B * (H / 2) * (W / 2) * (C / 4);
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 65536));
  ROMA_DT_SWITCH(dt, T, hipLaunchKernelGGL(maxpool_kernel<T>, grid, dim3(256), 0, s, (const T*)in, (T*)out, B, H, W, C));
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ DINOv2 patchify (im2col, 14x14 / stride 14)
template <typename TOUT>
__global__ __launch_bounds__(256) void im2col_patch14_kernel(const float* img, TOUT* out, int B, int H, int W, int Kpad) {
  const int th = H / 14, tw = W / 14;
  const long total = (long)B * th * tw * Kpad;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int k = (int)(idx % Kpad);
    long r = idx / Kpad;
    const int tx = (int)(r % tw);
    r /= tw;
    const int ty = (int)(r % th);
    const int b = (int)(r / th);
    float v = 0.f;
    if (k < 588) {
      const int c = k / 196, rem = k - c * 196, ky = rem / 14, kx = rem - ky * 14;
      v = img[((long)(b * 3 + c) * H + ty * 14 + ky) * W + tx * 14 + kx];
    }
    ElemIO<TOUT>::st(out + idx, v);
  }
}

int im2col_patch14_launch(const float* img, void* out, int B, int H, int W, int Kpad, int dt_out, hipStream_t s) {
  ROMA_REQUIRE(H % 14 == 0 && W % 14 == 0 && Kpad >= 588, "im2col_patch14: bad geometry");
  const long total = (long)B * (H / 14) * (W / 14) * Kpad;
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 65536));
  ROMA_DT_SWITCH(dt_out, T, hipLaunchKernelGGL(im2col_patch14_kernel<T>, grid, dim3(256), 0, s, img, (T*)out, B, H, W, Kpad));
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ token assembly (cls + pos-embed)
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const float* patch, const float* cls, const float* pos,
                                                              float* tokens, int B, int T, int D) {
  const int D4 = D / 4;
  const long total = (long)B * (T + 1) * D4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % D4) * 4;
    const long r = idx / D4;
    const int t = (int)(r % (T + 1));
    const int b = (int)(r / (T + 1));
    f32x4 v = (t == 0) ? *reinterpret_cast<const f32x4*>(cls + c)
                       : *reinterpret_cast<const f32x4*>(patch + ((long)b * T + (t - 1)) * D + c);
    v += *reinterpret_cast<const f32x4*>(pos + (long)t * D + c);
    *reinterpret_cast<f32x4*>(tokens + r * D + c) = v;
  }
}

int assemble_tokens_launch(const float* patch, const float* cls, const float* pos, float* tokens, int B, int T,
                           int D, hipStream_t s) {
  const long total = (long)B * (T + 1) * (D / 4);
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 65536));
  hipLaunchKernelGGL(assemble_tokens_kernel, grid, dim3(256), 0, s, patch, cls, pos, tokens, B, T, D);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ strided copy / convert
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void copy2d_kernel(const TI* in, long ldi, TO* out, long ldo, long rows, int cols) {
  const int c4n = cols / 4;
  const long total = rows * c4n;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % c4n) * 4;
    const long r = idx / c4n;
    ElemIO<TO>::st4(out + r * ldo + c, ElemIO<TI>::ld4(in + r * ldi + c));
  }
}

int copy2d_launch(const void* in, long ldi, int dt_in, void* out, long ldo, int dt_out, long rows, int cols,
                  hipStream_t s) {
  ROMA_REQUIRE(cols % 4 == 0 && ldi % 4 == 0 && ldo % 4 == 0, "copy2d: cols / strides must be multiples of 4");
  const long total = rows * (cols / 4);
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 65536));
  ROMA_DT_SWITCH(dt_in, TI, ROMA_DT_SWITCH(dt_out, TO, hipLaunchKernelGGL((copy2d_kernel<TI, TO>), grid, dim3(256), 0, s,
                                                                          (const TI*)in, ldi, (TO*)out, ldo, rows, cols)));
  ROMA_LAUNCH_CHECK();
  return 0;
}

// bfloat16 bits -> this build's 16-bit format (identity in the bf16 build): the hand-over of a ROMA_MIXED handle, whose
// DINOv2 ran in the bfloat16 library.  autocast does the same cast when the binary16 proj head consumes the bf16 features.
__global__ __launch_bounds__(256) void convert_from_bf16_kernel(const uint2* __restrict__ in, uint2* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const uint2 u = in[i];
    uint2 r;
    r.x = pack_bf16x2(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u));
    r.y = pack_bf16x2(__uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
    out[i] = r;
  }
}

int convert_from_bf16_launch(const void* in, void* out, long n, hipStream_t s) {
  ROMA_REQUIRE(n % 4 == 0 && n > 0, "convert_from_bf16: n must be a positive multiple of 4");
  const long n4 = n / 4;
  dim3 grid((unsigned)std::min<long>((n4 + 255) / 256, 65536));
  hipLaunchKernelGGL(convert_from_bf16_kernel, grid, dim3(256), 0, s, (const uint2*)in, (uint2*)out, n4);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ row L2 norms
template <typename T>
__global__ __launch_bounds__(256) void rownorm_kernel(const T* in, long ld, float* norms, long M, int C) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float s = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const f32x4 v = ElemIO<T>::ld4(in + row * ld + c);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  s = wave_sum(s);
  if (lane == 0) norms[row] = sqrtf(s);
}

int rownorm_launch(const void* in, long ld, int dt, float* norms, long M, int C, hipStream_t s) {
  ROMA_REQUIRE(C % 4 == 0, "rownorm: C must be a multiple of 4");
  dim3 grid((unsigned)((M + 3) / 4));
  ROMA_DT_SWITCH(dt, T, hipLaunchKernelGGL(rownorm_kernel<T>, grid, dim3(256), 0, s, (const T*)in, ld, norms, M, C));
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ GP Fourier basis (transposed)
// One copy per support image (blockIdx.y; copies `stride` floats apart): the GP stores F^T right behind each image's K_yy, and
// 16 back-to-back hipMemcpyAsync of one master copy cost more launches than recomputing 0.8 M cosines per image (round 5).
__global__ __launch_bounds__(256) void gp_basis_kernel(const float* w, const float* b, float* Ft, int Dg, int h, int wd,
                                                       int npad, long stride) {
  const long total = (long)Dg * npad;
  float* out = Ft + (long)blockIdx.y * stride;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int j = (int)(idx % npad);
    const int d = (int)(idx / npad);
    float v = 0.f;
    if (j < h * wd) {
      const int y = j / wd, x = j - y * wd;
      const float cx = pix_coord(x, wd), cy = pix_coord(y, h);
      const float z = w[d * 2 + 0] * cx + w[d * 2 + 1] * cy + b[d];
      v = cosf((float)(8.0 * 3.14159265358979323846) * z);
    }
    out[idx] = v;
  }
}

int gp_basis_launch(const float* w, const float* b, float* Ft, int Dg, int h, int wdt, int npad, hipStream_t s, int copies,
                    long stride) {
  const long total = (long)Dg * npad;
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 65536), (unsigned)std::max(copies, 1));
  hipLaunchKernelGGL(gp_basis_kernel, grid, dim3(256), 0, s, w, b, Ft, Dg, h, wdt, npad, stride);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ batched square transpose
__global__ __launch_bounds__(256) void transpose_kernel(const float* in, float* out, int n, long ld, long stride_in, long stride_out) {
  __shared__ float tile[32][33];
  const float* ib = in + (long)blockIdx.z * stride_in;
  float* ob = out + (long)blockIdx.z * stride_out;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
  for (int j = ty; j < 32; j += 8)
    if (y0 + j < n && x0 + tx < n) tile[j][tx] = ib[(long)(y0 + j) * ld + x0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (x0 + j < n && y0 + tx < n) ob[(long)(x0 + j) * ld + y0 + tx] = tile[tx][j];
}

int transpose_launch(const float* in, float* out, int n, long ld, int batch, hipStream_t s, long stride_in, long stride_out) {
  dim3 grid((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32), (unsigned)batch);
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, s, in, out, n, ld, stride_in > 0 ? stride_in : (long)n * ld,
                     stride_out > 0 ? stride_out : (long)n * ld);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ 64x64 Cholesky + triangular inverse
// ONE wave64 per diagonal block: lane i owns row i of the factor (and later column i of the inverse) in LDS.
// A single wave needs no barriers (its LDS operations complete in order), pivots / multipliers are LDS broadcast
// reads, rows are stride-65 so lane-parallel accesses are conflict free.  The previous 256-thread version spent
// 127 us per call on 192 __syncthreads(); the blocked Cholesky issues 25 such calls on the GP's critical path.
// (A fully unrolled register/readlane variant was correct but ~70 KB of straight-line code: instruction-fetch bound.)
// Round 4: TWO waves in a pipeline.  Row r of the inverse only needs columns <= r of the factor, and column j is final the
// moment the factorisation has finished its step j - so wave 1 runs the forward substitutions one row behind wave 0's column
// steps instead of after them (wave 0 publishes its progress in LDS with a release store behind a step's writes, wave 1 polls
// it with an acquire load in front of a row's reads), and all four
// waves share the 16 KB load and the 48 KB write-back.  53 -> ~33 us per call on the GP's launch-latency-bound chain (25 calls);
// arithmetic and its order unchanged: bit-identical results.
__global__ __launch_bounds__(256) void chol_diag_kernel(float* A, long ld, long strideA, float* Linv, float* LinvT,
                                                        int k, int nblk) {
  // the factorisation / inverse wave pair and the write-back live in chol_diag.h (shared with chol_col.hip)
  constexpr int S = CHOL_S;
  __shared__ __attribute__((aligned(16))) float L[64 * S];   // L[i][c]   (lane i owns row i)
  __shared__ __attribute__((aligned(16))) float LT[64 * S];  // LT[j][c] = L[c][j]   (broadcast source)
  __shared__ __attribute__((aligned(16))) float XT[64 * S];  // XT[c][t] = X[t][c]   (lane c owns row c)
  __shared__ int progress;  // last finished column step of the factorisation (workgroup-scope release / acquire)
  float* Ab = A + (long)blockIdx.x * strideA + ((long)k * 64) * ld + (long)k * 64;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = tid & 63;
  for (int idx = tid; idx < 64 * 16; idx += 256) {  // coalesced float4 loads
    const int row = idx >> 4, c4 = idx & 15;
    *reinterpret_cast<f32x4*>(&L[row * S + c4 * 4]) = *reinterpret_cast<const f32x4*>(Ab + (long)row * ld + c4 * 4);
  }
  if (tid == 0) progress = -1;
  __syncthreads();
  if (wave == 0) chol_diag_factor_wave(L, LT, &progress, i);
  else if (wave == 1) chol_diag_inverse_wave(L, XT, &progress, i);
  __syncthreads();
  chol_diag_writeback(L, XT, Ab, ld, Linv + ((long)blockIdx.x * nblk + k) * 4096, LinvT + ((long)blockIdx.x * nblk + k) * 4096,
                      tid, 256);
}

int chol_diag_launch(float* A, long ld, long strideA, float* Linv, float* LinvT, int k, int nblk, int batch,
                     hipStream_t s) {
  hipLaunchKernelGGL(chol_diag_kernel, dim3((unsigned)batch), dim3(256), 0, s, A, ld, strideA, Linv, LinvT, k, nblk);
  ROMA_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void pad_identity_kernel(float* A, long ld, long strideA, int n, int npad) {
  float* Ab = A + (long)blockIdx.y * strideA;
  const long total = (long)npad * npad;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int i = (int)(idx / npad), j = (int)(idx % npad);
    if (i >= n || j >= n) Ab[(long)i * ld + j] = (i == j) ? 1.f : 0.f;
  }
}

int pad_identity_launch(float* A, long ld, long strideA, int n, int npad, int batch, hipStream_t s) {
  if (npad == n) return 0;
  const long total = (long)npad * npad;
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 4096), (unsigned)batch);
  hipLaunchKernelGGL(pad_identity_kernel, grid, dim3(256), 0, s, A, ld, strideA, n, npad);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ cls_to_flow_refine
__global__ __launch_bounds__(256) void cls_to_flow_kernel(const float* logits, long ld, float* flow, float* cert, long M) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* lr = logits + row * ld;
  float mx = -INFINITY;
  int arg = 0;
  f32x4 v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    v[i] = *reinterpret_cast<const f32x4*>(lr + (i * 64 + lane) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (v[i][j] > mx) {
        mx = v[i][j];
        arg = (i * 64 + lane) * 4 + j;
      }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float om = __shfl_xor(mx, off);
    const int oa = __shfl_xor(arg, off);
    if (om > mx || (om == mx && oa < arg)) {
      mx = om;
      arg = oa;
    }
  }
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) se += expf(v[i][j] - mx);
  se = wave_sum(se);
  if (lane == 0) {
    const int idx5[5] = {arg - 1, arg, arg + 1, arg - 64, arg + 64};
    float fx = 0.f, fy = 0.f, tot = 0.f;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int c = min(max(idx5[t], 0), 4095);
      const float p = expf(lr[c] - mx) / se;
      fx += p * pix_coord(c & 63, 64);
      fy += p * pix_coord(c >> 6, 64);
      tot += p;
    }
    flow[row * 2 + 0] = fx / tot;
    flow[row * 2 + 1] = fy / tot;
    cert[row] = lr[4096];
  }
}

int cls_to_flow_launch(const float* logits, long ld, float* flow, float* cert, long M, hipStream_t s) {
  ROMA_REQUIRE(ld % 4 == 0 && ld >= 4097, "cls_to_flow: bad leading dimension");
  dim3 grid((unsigned)((M + 3) / 4));
  hipLaunchKernelGGL(cls_to_flow_kernel, grid, dim3(256), 0, s, logits, ld, flow, cert, M);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ bilinear resize (align_corners=False)
__device__ inline void bilinear_src(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = src - (float)i0;
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* in, float* out, int B, int Hin, int Win, int Hout,
                                                              int Wout, int nc) {
  const float sh = (float)Hin / (float)Hout, sw = (float)Win / (float)Wout;
  const long total = (long)B * Hout * Wout;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int x = (int)(idx % Wout);
    long r = idx / Wout;
    const int y = (int)(r % Hout);
    const int b = (int)(r / Hout);
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_src(y, sh, Hin, y0, y1, ly);
    bilinear_src(x, sw, Win, x0, x1, lx);
    const float* ib = in + (long)b * Hin * Win * nc;
    for (int c = 0; c < nc; ++c) {
      const float v00 = ib[((long)y0 * Win + x0) * nc + c], v01 = ib[((long)y0 * Win + x1) * nc + c];
      const float v10 = ib[((long)y1 * Win + x0) * nc + c], v11 = ib[((long)y1 * Win + x1) * nc + c];
      out[idx * nc + c] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    }
  }
}

int resize_bilinear_launch(const float* in, float* out, int B, int Hin, int Win, int Hout, int Wout, int nc,
                           hipStream_t s) {
  const long total = (long)B * Hout * Wout;
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 65536));
  hipLaunchKernelGGL(resize_bilinear_kernel, grid, dim3(256), 0, s, in, out, B, Hin, Win, Hout, Wout, nc);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ final epilogue (matcher.py:839-850, 891-929)
__global__ __launch_bounds__(256) void final_epilogue_kernel(const FinalArgs a) {
  const int Wout = a.symmetric ? 2 * a.W : a.W;
  const long total = (long)a.B * a.H * Wout;
  const float sh = a.cert16 ? (float)a.h16 / (float)a.H : 0.f, sw = a.cert16 ? (float)a.w16 / (float)a.W : 0.f;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int xo = (int)(idx % Wout);
    long r = idx / Wout;
    const int y = (int)(r % a.H);
    const int bo = (int)(r / a.H);
    const int half = xo / a.W, x = xo - half * a.W;
    const int dp = bo + half * a.B;
    const long src = ((long)dp * a.H + y) * a.W + x;
    float fx = a.flow[src * 2 + 0], fy = a.flow[src * 2 + 1];
    float c = a.cert[src];
    if (a.cert16) {
      int y0, y1, x0, x1;
      float ly, lx;
      bilinear_src(y, sh, a.h16, y0, y1, ly);
      bilinear_src(x, sw, a.w16, x0, x1, lx);
      const float* cb = a.cert16 + (long)dp * a.h16 * a.w16;
      const float low = (1.f - ly) * ((1.f - lx) * cb[y0 * a.w16 + x0] + lx * cb[y0 * a.w16 + x1]) +
                        ly * ((1.f - lx) * cb[y1 * a.w16 + x0] + lx * cb[y1 * a.w16 + x1]);
      c -= (low < 0.f) ? 0.5f * low : 0.f;
    }
    c = 1.f / (1.f + expf(-c));
    if (fabsf(fx) > 1.f || fabsf(fy) > 1.f) c = 0.f;
    fx = fminf(fmaxf(fx, -1.f), 1.f);
    fy = fminf(fmaxf(fy, -1.f), 1.f);
    const float gx = pix_coord(x, a.W), gy = pix_coord(y, a.H);
    f32x4 o;
    if (half == 0) o = f32x4{gx, gy, fx, fy};
    else o = f32x4{fx, fy, gx, gy};
    *reinterpret_cast<f32x4*>(a.warp + idx * 4) = o;
    a.certainty[idx] = c;
  }
}

int final_epilogue_launch(const FinalArgs& a, hipStream_t s) {
  const long total = (long)a.B * a.H * (a.symmetric ? 2 * a.W : a.W);
  dim3 grid((unsigned)std::min<long>((total + 255) / 256, 65536));
  hipLaunchKernelGGL(final_epilogue_kernel, grid, dim3(256), 0, s, a);
  ROMA_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- determinism trace (debug)
// Order-independent 64-bit checksum of a buffer: XOR over the words of mix(word, index).  Any single changed bit changes
// the sum; the result does not depend on how threads are scheduled.  Used by Model::trace (option "trace") to find the
// FIRST stage whose output differs between two runs of the same inputs.
__global__ __launch_bounds__(256) void checksum_kernel(const uint32_t* p, long nwords, unsigned long long* out) {
  unsigned long long h = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (long)gridDim.x * 256) {
    unsigned long long x = ((unsigned long long)p[i] << 32) ^ (unsigned long long)(i * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    h ^= x;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)h, off), hi = __shfl_xor((unsigned)(h >> 32), off);
    h ^= ((unsigned long long)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0 && h) atomicXor(out, h);
}

// diagnostic variant: only columns [c0, c1) of a [rows][ld] matrix of 16-bit elements
__global__ __launch_bounds__(256) void checksum_cols_kernel(const unsigned short* p, long rows, int ld, int c0, int c1,
                                                            unsigned long long* out) {
  unsigned long long h = 0;
  const int nc = c1 - c0;
  const long n = rows * nc;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / nc;
    const int c = c0 + (int)(i - r * nc);
    unsigned long long x = ((unsigned long long)p[r * ld + c] << 32) ^ (unsigned long long)(i * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    h ^= x;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)h, off), hi = __shfl_xor((unsigned)(h >> 32), off);
    h ^= ((unsigned long long)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0 && h) atomicXor(out, h);
}

int checksum_cols_launch(const void* p, long rows, int ld, int c0, int c1, unsigned long long* out, hipStream_t s) {
  if (rows <= 0 || c1 <= c0) return 0;
  const unsigned grid = (unsigned)std::min<long>((rows * (c1 - c0) + 255) / 256, 1024);
  hipLaunchKernelGGL(checksum_cols_kernel, dim3(grid), dim3(256), 0, s, static_cast<const unsigned short*>(p), rows, ld, c0, c1, out);
  ROMA_LAUNCH_CHECK();
  return 0;
}

int checksum_launch(const void* p, size_t bytes, unsigned long long* out, hipStream_t s) {
  const long nwords = (long)(bytes / 4);
  if (nwords <= 0) return 0;
  const unsigned grid = (unsigned)std::min<long>((nwords + 255) / 256, 1024);
  hipLaunchKernelGGL(checksum_kernel, dim3(grid), dim3(256), 0, s, static_cast<const uint32_t*>(p), nwords, out);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
