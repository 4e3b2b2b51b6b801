// elementwise.h plus the device helpers that its four sources share.  Private to them: callers include elementwise.h only.
#pragma once
#include "elementwise.h"
#include "gemm.h"  // DT_*
#define ROMA_DT_SWITCH(dt, T, ...)            \
  if ((dt) == DT_F32) { using T = float; __VA_ARGS__; } else { using T = bf16_t; __VA_ARGS__; }

namespace roma {

typedef __attribute__((ext_vector_type(2))) float f32x2;

// torch.linspace(-1+1/n, 1-1/n, n)[i] in f32 (symmetric two-sided evaluation like ATen)
__device__ inline float pix_coord(int i, int n) {
  const float start = (float)(-1.0 + 1.0 / n), end = (float)(1.0 - 1.0 / n);
  if (n == 1) return start;
  const float step = (end - start) / (float)(n - 1);
  return (i < n / 2) ? start + step * (float)i : end - step * (float)(n - 1 - i);
}

// 16 bytes per access: 4 f32 / 8 h16 of one channels-last row (the vectorised refiner-input and out_conv kernels)
template <typename T> struct VecIO;
template <> struct VecIO<float> {
  static constexpr int CV = 4;
  typedef f32x4 Raw;  // 16 bytes as loaded; cvt() turns them into CV floats (the same values ld() delivers)
  __device__ static inline Raw ldraw(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  __device__ static inline void cvt(const Raw& x, float* v) { v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3]; }
  __device__ static inline void ld(const float* p, float* v) { cvt(ldraw(p), v); }
  __device__ static inline void st(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct VecIO<bf16_t> {
  static constexpr int CV = 8;
  typedef uint4 Raw;
  __device__ static inline Raw ldraw(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
  __device__ static inline void cvt(const Raw& u, float* v) {
    v[0] = h16_lo(u.x); v[1] = h16_hi(u.x);
    v[2] = h16_lo(u.y); v[3] = h16_hi(u.y);
    v[4] = h16_lo(u.z); v[5] = h16_hi(u.z);
    v[6] = h16_lo(u.w); v[7] = h16_hi(u.w);
  }
  __device__ static inline void ld(const bf16_t* p, float* v) { cvt(ldraw(p), v); }
  __device__ static inline void st(bf16_t* p, const float* v) {
    uint4 u;
    u.x = pack_bf16x2(v[0], v[1]);
    u.y = pack_bf16x2(v[2], v[3]);
    u.z = pack_bf16x2(v[4], v[5]);
    u.w = pack_bf16x2(v[6], v[7]);
    *reinterpret_cast<uint4*>(p) = u;
  }
};

}  // namespace roma
