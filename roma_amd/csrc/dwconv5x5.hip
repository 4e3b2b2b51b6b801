// Depthwise 5x5 + BN(folded) + ReLU, register-prefetch form (elementwise.h).  A stencil source: v_pk_fma_f32 on purpose (PK_SRCS).
#include "elementwise_device.h"

namespace roma {

// Rolling-window form.  The stencil is NOT HBM-bound on MI355X when written naively: 25 MAC per 2-byte element put
// it on the VALU / vector-L1 path (a first version re-loaded the 25 weight vectors and 6 input rows per 8 outputs
// and ran at 1.4 TB/s with the texture path saturated).  Here one thread owns 4 channels x 4 x-positions and walks a
// strip of rows top to bottom:
//   * its 25 x 4 weights stay in registers for the whole strip (one load per thread, not per output),
//   * each input row is loaded ONCE (8 vectors) and feeds the 5 output rows it touches (5 rolling accumulator
//     slots that are rotated after every row), i.e. 200 packed-f32 FMAs (v_pk_fma_f32) per 8 loads,
//   * the next input row is prefetched while the current one is multiplied.
// Workgroups are remapped so each XCD owns a contiguous band of strips (private L2 sees the 4-row halo once).
template <typename T> struct RawVec;
template <> struct RawVec<float> {
  typedef f32x4 raw;
  __device__ static inline raw ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  __device__ static inline raw mask(raw r, uint32_t m) {  // bitwise AND keeps the load unconditional (no branch)
    return f32x4{__uint_as_float(__float_as_uint(r[0]) & m), __uint_as_float(__float_as_uint(r[1]) & m),
                 __uint_as_float(__float_as_uint(r[2]) & m), __uint_as_float(__float_as_uint(r[3]) & m)};
  }
  __device__ static inline void cvt(raw r, f32x2& a, f32x2& b) { a = f32x2{r[0], r[1]}; b = f32x2{r[2], r[3]}; }
  __device__ static inline void st(float* p, f32x2 a, f32x2 b) { *reinterpret_cast<f32x4*>(p) = f32x4{a[0], a[1], b[0], b[1]}; }
};
template <> struct RawVec<bf16_t> {
  typedef uint2 raw;
  __device__ static inline raw ld(const bf16_t* p) { return *reinterpret_cast<const uint2*>(p); }
  __device__ static inline raw mask(raw r, uint32_t m) { return make_uint2(r.x & m, r.y & m); }
  __device__ static inline void cvt(raw r, f32x2& a, f32x2& b) {
    a = f32x2{h16_lo(r.x), h16_hi(r.x)};
    b = f32x2{h16_lo(r.y), h16_hi(r.y)};
  }
  __device__ static inline void st(bf16_t* p, f32x2 a, f32x2 b) {
    uint2 u;
    u.x = pack_bf16x2(a[0], a[1]);
    u.y = pack_bf16x2(b[0], b[1]);
    *reinterpret_cast<uint2*>(p) = u;
  }
};

template <typename T>
__global__ __launch_bounds__(256, 2) void dwconv5x5_kernel(const T* in, T* out, const float* w, const float* bias, int B,
                                                           int H, int W, int Cp, int SY, int GC, int nchunk, int nxg,
                                                           int nblocks) {
  typedef typename RawVec<T>::raw raw_t;
  extern __shared__ __attribute__((aligned(16))) float wsm[];  // [25][GC*4] weights + [GC*4] bias of this channel chunk
  const int per_xcd = (nblocks + 7) / 8;
  const long lb = (long)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  if (lb >= nblocks) return;
  const int chunk = (int)(lb % nchunk);
  long r = lb / nchunk;
  const int xg = (int)(r % nxg);
  r /= nxg;
  const int yt = (H + SY - 1) / SY;
  const int ys = (int)(r % yt) * SY;
  const int b = (int)(r / yt);
  const int XQ = 256 / GC;
  const int cg = threadIdx.x % GC, xq = threadIdx.x / GC;
  const int c0 = chunk * GC * 4;
  constexpr int cw = 256;  // fixed LDS row stride: weight reads become base + immediate offset
  // stage this chunk's 25 x (GC*4) weights + bias as float4s; all loads are issued before the first LDS write
  // (a dword-at-a-time loop serialised 26 dependent global loads = ~40 us per workgroup)
  {
    const int q4 = GC;                   // float4 columns actually used per row
    const int nvec = 26 * q4;            // <= 26 * 64
    f32x4 tmp[7];
#pragma unroll
    for (int it = 0; it < 7; ++it) {
      const int i = threadIdx.x + 256 * it;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (i < nvec) {
        const int t = i / q4, cq = i - t * q4;
        const int ch = c0 + cq * 4;
        if (ch < Cp) v = *reinterpret_cast<const f32x4*>(t < 25 ? w + (long)t * Cp + ch : bias + ch);
      }
      tmp[it] = v;
    }
#pragma unroll
    for (int it = 0; it < 7; ++it) {
      const int i = threadIdx.x + 256 * it;
      if (i < nvec) {
        const int t = i / q4, cq = i - t * q4;
        *reinterpret_cast<f32x4*>(&wsm[t * cw + cq * 4]) = tmp[it];
      }
    }
  }
  __syncthreads();
  const int c = c0 + cg * 4;
  const int xb = (xg * XQ + xq) * 4;
  if (xq >= XQ || c >= Cp || xb >= W) return;
  const int sy = min(SY, H - ys);

  const f32x4 bx = *reinterpret_cast<const f32x4*>(&wsm[25 * cw + cg * 4]);
  const f32x2 bias0 = f32x2{bx[0], bx[1]}, bias1 = f32x2{bx[2], bx[3]};
  f32x2 acc[5][4][2];
#pragma unroll
  for (int s5 = 0; s5 < 5; ++s5)
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      acc[s5][px][0] = bias0;
      acc[s5][px][1] = bias1;
    }
  bool colok[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) colok[j] = (xb - 2 + j >= 0) && (xb - 2 + j < W);
  long colofs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) colofs[j] = (long)min(max(xb - 2 + j, 0), W - 1) * Cp;
  const T* base = in + ((long)b * H * W) * Cp + c;
  T* obase = out + ((long)b * H * W) * Cp + c;

// branch-free row load: out-of-image taps read a clamped (valid) address and are zeroed by a select afterwards
#define ROMA_DW_LOAD_ROW(TT, DST)                                                                         \
  {                                                                                                       \
    const int yy_ = ys - 2 + (TT);                                                                        \
    const bool rok_ = yy_ >= 0 && yy_ < H;                                                                \
    const T* rowp_ = base + (long)min(max(yy_, 0), H - 1) * W * Cp;                                       \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                       \
      DST[j] = RawVec<T>::mask(RawVec<T>::ld(rowp_ + colofs[j]), (rok_ && colok[j]) ? 0xffffffffu : 0u);  \
    }                                                                                                     \
  }

  // acc[k] holds output row o = t - 4 + k while input row t is processed (tap row ky = 4 - k)
  raw_t cur[8], nxt[8];
  ROMA_DW_LOAD_ROW(0, cur);
#pragma nounroll
  for (int t = 0; t < sy + 4; ++t) {
    ROMA_DW_LOAD_ROW(t + 1, nxt);
    f32x2 v[8][2];
#pragma unroll
    for (int j = 0; j < 8; ++j) RawVec<T>::cvt(cur[j], v[j][0], v[j][1]);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int ky = 4 - k;
#pragma unroll
      for (int kx = 0; kx < 5; ++kx) {
        const f32x4 wx = *reinterpret_cast<const f32x4*>(&wsm[(ky * 5 + kx) * cw + cg * 4]);
        const f32x2 w0 = f32x2{wx[0], wx[1]}, w1 = f32x2{wx[2], wx[3]};
#pragma unroll
        for (int px = 0; px < 4; ++px) {
          acc[k][px][0] = v[px + kx][0] * w0 + acc[k][px][0];
          acc[k][px][1] = v[px + kx][1] * w1 + acc[k][px][1];
        }
      }
    }
    const int o = t - 4;
    if (o >= 0) {
      T* orow = obase + ((long)(ys + o) * W + xb) * Cp;
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        if (xb + px < W) {
          f32x2 a0 = acc[0][px][0], a1 = acc[0][px][1];
          a0 = f32x2{fmaxf(a0[0], 0.f), fmaxf(a0[1], 0.f)};
          a1 = f32x2{fmaxf(a1[0], 0.f), fmaxf(a1[1], 0.f)};
          RawVec<T>::st(orow + (long)px * Cp, a0, a1);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        acc[k][px][0] = acc[k + 1][px][0];
        acc[k][px][1] = acc[k + 1][px][1];
      }
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      acc[4][px][0] = bias0;
      acc[4][px][1] = bias1;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) cur[j] = nxt[j];
  }
}
#undef ROMA_DW_LOAD_ROW

int dwconv5x5_launch(const void* in, void* out, const float* w, const float* bias, int B, int H, int W, int Cp,
                     int dt, hipStream_t s) {
  ROMA_REQUIRE(Cp % 4 == 0, "dwconv5x5: padded channel count must be a multiple of 4");
  ROMA_REQUIRE(in != out, "dwconv5x5: in and out must not alias");
  {  // wide 16-bit problems: the wave-private LDS-DMA ring form (dwconv_ring.hip), bit-identical
    const int rc = dwconv5x5_ring_try_launch(in, out, w, bias, B, H, W, Cp, dt, s);
    if (rc <= 0) return rc;
  }
  const int CG = Cp / 4;
  const int nchunk = (CG + 63) / 64;
  const int GC = (CG + nchunk - 1) / nchunk;  // channel groups (of 4) per workgroup, <= 64
  const int XQ = 256 / GC;                    // x tiles (of 4 pixels) per workgroup
  const int nxg = ((W + 3) / 4 + XQ - 1) / XQ;
  // strip height: SY + 4 input rows are read per strip, so 36-row strips cost 11 % extra rows against 25 % for
  // 16-row strips - as long as there are still enough workgroups to fill 256 CUs x 2
  int SY = 36;
  if ((long)B * ((H + 35) / 36) * nxg * nchunk < 1024) SY = 16;
  const long nb = (long)B * ((H + SY - 1) / SY) * nxg * nchunk;
  const int nblocks = (int)nb;
  dim3 grid((unsigned)(((nblocks + 7) / 8) * 8));
  const size_t lds = (size_t)26 * 256 * sizeof(float);  // fixed 256-float rows (see kernel)
  ProfScope ps(dt == DT_F32 ? "dwconv5x5_kernel<f32>" : "dwconv5x5_kernel<" ROMA_H16_NAME ">",
               2.0 * (double)B * H * W * Cp * (dt == DT_F32 ? 4.0 : 2.0), "byte", s);
  ROMA_DT_SWITCH(dt, T, hipLaunchKernelGGL(dwconv5x5_kernel<T>, grid, dim3(256), lds, s, (const T*)in, (T*)out, w, bias, B, H, W, Cp, SY, GC, nchunk, nxg, nblocks));
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
