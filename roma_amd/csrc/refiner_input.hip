// ConvRefiner input d = [x | grid_sample(y, flow) | disp_emb | . | 0] (see elementwise.h): four kernels, one launcher.
#include <algorithm>
#include <stdio.h>
#include "elementwise_device.h"
#include "tuning.h"

namespace roma {

// grid_sample(bilinear, align_corners=False) at (wx, wy): top-left tap (x0, y0), weights of taps (+0,+0) (+1,+0) (+0,+1) (+1,+1)
__device__ __forceinline__ void bilinear_taps(float wx, float wy, int W, int H, int& x0, int& y0, float (&wgt)[4]) {
  float ix = ((wx + 1.f) * W - 1.f) * 0.5f, iy = ((wy + 1.f) * H - 1.f) * 0.5f;
  ix = fminf(fmaxf(ix, -1.0e6f), 1.0e6f);  // clamped: the conversion to int below is defined for any flow
  iy = fminf(fmaxf(iy, -1.0e6f), 1.0e6f);
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  x0 = (int)fx0; y0 = (int)fy0;
  const float tx = ix - fx0, ty = iy - fy0;
  wgt[0] = (1.f - tx) * (1.f - ty); wgt[1] = tx * (1.f - ty); wgt[2] = (1.f - tx) * ty; wgt[3] = tx * ty;
}

// one wave per pixel (what the vector kernel below does not take: a buffer that is not 16-byte aligned)
template <typename T>
__global__ __launch_bounds__(256) void refiner_input_kernel(const RefinerInputArgs a) {
  const int lane = threadIdx.x & 63;
  const long HW = (long)a.H * a.W;
  const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= (long)a.B * HW) return;
  const int b = (int)(pix / HW);
  const long p = pix - (long)b * HW;
  const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
  const T* feat = reinterpret_cast<const T*>(a.feat);
  const T* fq = feat + ((long)b * HW + p) * a.ldf;
  const int simg = (b + a.shift) % a.nimg;
  const T* fs = feat + (long)simg * HW * a.ldf;
  T* d = reinterpret_cast<T*>(a.d) + pix * a.ldd;
  const float wx = a.flow[pix * 2 + 0], wy = a.flow[pix * 2 + 1];
  int x0, y0;
  float wgt[4];
  bilinear_taps(wx, wy, a.W, a.H, x0, y0, wgt);
  bool ok[4];
  long off[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
    ok[t] = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
    off[t] = ((long)yy * a.W + xx) * a.ldf;
  }
  for (int c = lane * 4; c < a.C; c += 256) {
    ElemIO<T>::st4(d + c, ElemIO<T>::ld4(fq + c));
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (ok[t]) {
        const f32x4 v = ElemIO<T>::ld4(fs + off[t] + c);
        acc += wgt[t] * v;
      }
    ElemIO<T>::st4(d + a.C + c, acc);
  }
  const float dx = a.disp_scale * (wx - pix_coord(x, a.W)), dy = a.disp_scale * (wy - pix_coord(y, a.H));
  for (int e = lane; e < a.E; e += 64) {
    const float v = a.emb_w[e * 2 + 0] * dx + a.emb_w[e * 2 + 1] * dy + a.emb_b[e];
    ElemIO<T>::st(d + 2 * a.C + e, v);
  }
  for (long c = 2 * a.C + a.E + a.Kcorr + lane; c < a.ldd; c += 64) ElemIO<T>::st(d + c, 0.f);
}

// small / odd channel counts (stride-1 refiner: C = 9): one thread per (pixel, padded channel slot)
template <typename T>
__global__ __launch_bounds__(256) void refiner_input_small_kernel(const RefinerInputArgs a) {
  const long HW = (long)a.H * a.W;
  const int slots = (int)a.ldd;
  const long total = (long)a.B * HW * slots;
  const T* feat = reinterpret_cast<const T*>(a.feat);
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % slots);
    const long pix = idx / slots;
    const int b = (int)(pix / HW);
    const long p = pix - (long)b * HW;
    T* d = reinterpret_cast<T*>(a.d) + pix * a.ldd;
    if (c < a.C) {
      ElemIO<T>::st(d + c, ElemIO<T>::ld(feat + ((long)b * HW + p) * a.ldf + c));
    } else if (c < 2 * a.C) {
      const int cc = c - a.C;
      const int simg = (b + a.shift) % a.nimg;
      const T* fs = feat + (long)simg * HW * a.ldf;
      const float wx = a.flow[pix * 2 + 0], wy = a.flow[pix * 2 + 1];
      int x0, y0;
      float wgt[4];
      bilinear_taps(wx, wy, a.W, a.H, x0, y0, wgt);
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W)
          acc += wgt[t] * ElemIO<T>::ld(fs + ((long)yy * a.W + xx) * a.ldf + cc);
      }
      ElemIO<T>::st(d + c, acc);
    } else if (c < 2 * a.C + a.E) {
      const int e = c - 2 * a.C;
      const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
      const float dx = a.disp_scale * (a.flow[pix * 2 + 0] - pix_coord(x, a.W));
      const float dy = a.disp_scale * (a.flow[pix * 2 + 1] - pix_coord(y, a.H));
      ElemIO<T>::st(d + c, a.emb_w[e * 2 + 0] * dx + a.emb_w[e * 2 + 1] * dy + a.emb_b[e]);
    } else if (c >= 2 * a.C + a.E + a.Kcorr) {
      ElemIO<T>::st(d + c, 0.f);
    }
  }
}

// stride-1 refiner (C = 9, E = 6, 24 output channels): one thread per pixel, whole rows as 16-byte vectors
template <typename T, int C, int E>
__global__ __launch_bounds__(256) void refiner_input_pix_kernel(const RefinerInputArgs a) {
  constexpr int LDF = 16, LDD = 24;
  const long HW = (long)a.H * a.W;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (long)a.B * HW) return;
  const int b = (int)(pix / HW);
  const long p = pix - (long)b * HW;
  const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
  const T* feat = reinterpret_cast<const T*>(a.feat);
  const T* fq = feat + ((long)b * HW + p) * LDF;
  const int simg = (b + a.shift) % a.nimg;
  const T* fs = feat + (long)simg * HW * LDF;
  if constexpr (sizeof(T) == 2) {
    // bf16: 16-byte accesses - a pixel's 16 feature channels are two loads (were three 8-byte ones), its 24 output channels
    // three stores (were six): this kernel is bound by the number of memory instructions, not by bytes
    static_assert(C <= 16 && 2 * C + E <= LDD && LDD == 24 && LDF == 16, "layout");
    float q[16], xh[16];
    VecIO<T>::ld(fq, q);
    VecIO<T>::ld(fq + 8, q + 8);
#pragma unroll
    for (int j = 0; j < 16; ++j) xh[j] = 0.f;
    const float wx = a.flow[pix * 2 + 0], wy = a.flow[pix * 2 + 1];
    int x0, y0;
    float wgt[4];
    bilinear_taps(wx, wy, a.W, a.H, x0, y0, wgt);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
      if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
        const T* r = fs + ((long)yy * a.W + xx) * LDF;
        float v[16];
        VecIO<T>::ld(r, v);
        VecIO<T>::ld(r + 8, v + 8);
#pragma unroll
        for (int j = 0; j < C; ++j) xh[j] += wgt[t] * v[j];
      }
    }
    const float dx = a.disp_scale * (wx - pix_coord(x, a.W)), dy = a.disp_scale * (wy - pix_coord(y, a.H));
    float o[LDD];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      o[c] = q[c];
      o[C + c] = xh[c];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) o[2 * C + e] = a.emb_w[e * 2 + 0] * dx + a.emb_w[e * 2 + 1] * dy + a.emb_b[e];
#pragma unroll
    for (int c = 2 * C + E; c < LDD; ++c) o[c] = 0.f;
    T* d = reinterpret_cast<T*>(a.d) + pix * LDD;
#pragma unroll
    for (int c8 = 0; c8 < LDD / 8; ++c8) VecIO<T>::st(d + c8 * 8, o + c8 * 8);
    return;
  }
  float q[12], xh[12];
#pragma unroll
  for (int c4 = 0; c4 < 3; ++c4) {
    const f32x4 v = ElemIO<T>::ld4(fq + c4 * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q[c4 * 4 + j] = v[j];
      xh[c4 * 4 + j] = 0.f;
    }
  }
  const float wx = a.flow[pix * 2 + 0], wy = a.flow[pix * 2 + 1];
  int x0, y0;
  float wgt[4];
  bilinear_taps(wx, wy, a.W, a.H, x0, y0, wgt);
  // (guarded taps on purpose: the branch-free form that helps the vector kernel below - clamped address + select - was
  //  measured SLOWER here, 0.94 vs 0.78 ms per step)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
    if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
      const T* r = fs + ((long)yy * a.W + xx) * LDF;
#pragma unroll
      for (int c4 = 0; c4 < 3; ++c4) {
        const f32x4 v = ElemIO<T>::ld4(r + c4 * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) xh[c4 * 4 + j] += wgt[t] * v[j];
      }
    }
  }
  const float dx = a.disp_scale * (wx - pix_coord(x, a.W)), dy = a.disp_scale * (wy - pix_coord(y, a.H));
  float o[LDD];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    o[c] = q[c];
    o[C + c] = xh[c];
  }
#pragma unroll
  for (int e = 0; e < E; ++e) o[2 * C + e] = a.emb_w[e * 2 + 0] * dx + a.emb_w[e * 2 + 1] * dy + a.emb_b[e];
#pragma unroll
  for (int c = 2 * C + E; c < LDD; ++c) o[c] = 0.f;
  T* d = reinterpret_cast<T*>(a.d) + pix * LDD;
#pragma unroll
  for (int c4 = 0; c4 < LDD / 4; ++c4) ElemIO<T>::st4(d + c4 * 4, f32x4{o[c4 * 4], o[c4 * 4 + 1], o[c4 * 4 + 2], o[c4 * 4 + 3]});
}

// refiner input, vectorised: LPP lanes (a power of two) share one pixel, 64/LPP pixels per wave, 16 bytes per lane
// per access.  The wave-per-pixel kernel above left 48 of 64 lanes idle at C = 64 (stride-2 refiner, 4.2 M pixels).
template <typename T>
__global__ __launch_bounds__(256) void refiner_input_vec_kernel(const RefinerInputArgs a, int lpp) {
  constexpr int CV = VecIO<T>::CV;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (lpp - 1), pw = lane / lpp, ppw = 64 / lpp;
  const long HW = (long)a.H * a.W;
  const long pix = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * ppw + pw;
  if (pix >= (long)a.B * HW) return;
  const int b = (int)(pix / HW);
  const long p = pix - (long)b * HW;
  const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
  const T* feat = reinterpret_cast<const T*>(a.feat);
  const T* fq = feat + ((long)b * HW + p) * a.ldf;
  const int simg = (b + a.shift) % a.nimg;
  const T* fs = feat + (long)simg * HW * a.ldf;
  T* d = reinterpret_cast<T*>(a.d) + pix * a.ldd;
  const float wx = a.flow[pix * 2 + 0], wy = a.flow[pix * 2 + 1];
  int x0, y0;
  float wgt[4];
  bilinear_taps(wx, wy, a.W, a.H, x0, y0, wgt);
  bool ok[4];
  long off[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
    ok[t] = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;  // zeros padding: out-of-image taps are dropped (select below)
    off[t] = ((long)min(max(yy, 0), a.H - 1) * a.W + min(max(xx, 0), a.W - 1)) * a.ldf;  // always a valid address
  }
  for (int c = sub * CV; c < a.C; c += lpp * CV) {
    *reinterpret_cast<uint4*>(d + c) = *reinterpret_cast<const uint4*>(fq + c);
    float r[CV];
#pragma unroll
    for (int j = 0; j < CV; ++j) r[j] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {  // branch-free: the four tap loads of a channel piece are in flight together
      float tv[CV];
      VecIO<T>::ld(fs + off[t] + c, tv);
#pragma unroll
      for (int j = 0; j < CV; ++j) r[j] = ok[t] ? r[j] + wgt[t] * tv[j] : r[j];
    }
    VecIO<T>::st(d + a.C + c, r);
  }
  const float dx = a.disp_scale * (wx - pix_coord(x, a.W)), dy = a.disp_scale * (wy - pix_coord(y, a.H));
  for (int e = sub; e < a.E; e += lpp) {
    const float v = a.emb_w[e * 2 + 0] * dx + a.emb_w[e * 2 + 1] * dy + a.emb_b[e];
    ElemIO<T>::st(d + 2 * a.C + e, v);
  }
  for (long c = 2 * a.C + a.E + a.Kcorr + sub; c < a.ldd; c += lpp) ElemIO<T>::st(d + c, 0.f);
}

int refiner_input_launch(const RefinerInputArgs& a, hipStream_t s) {
  const long npix = (long)a.B * a.H * a.W;
  // grid_sample warp + concat writer (matcher.py:132-148,166).  Algorithmic bytes: x and the sampled y
  // read once (2 s C), the flow (8), the written row of d without the correlation slice another kernel fills
  const double es = a.dt == DT_F32 ? 4.0 : 2.0;
  char pname[64];
  snprintf(pname, sizeof pname, "refiner_input_warp<C=%d,%s>", a.C, a.dt == DT_F32 ? "f32" : ROMA_H16_NAME);
  ProfScope ps(pname, (double)npix * (2.0 * a.C * es + 8.0 + (double)(a.ldd - a.Kcorr) * es), "byte", s);
  if (a.C == 9 && a.E == 6 && a.Kcorr == 0 && a.ldf == 16 && a.ldd == 24) {
    dim3 grid((unsigned)((npix + 255) / 256));
    ROMA_DT_SWITCH(a.dt, T, hipLaunchKernelGGL((refiner_input_pix_kernel<T, 9, 6>), grid, dim3(256), 0, s, a));
    ROMA_LAUNCH_CHECK();
    return 0;
  }
  if (a.C % 4 != 0 || a.C < 32) {
    const long total = npix * a.ldd;
    dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1 << 20));
    ROMA_DT_SWITCH(a.dt, T, hipLaunchKernelGGL(refiner_input_small_kernel<T>, grid, dim3(256), 0, s, a));
    ROMA_LAUNCH_CHECK();
    return 0;
  }
  ROMA_REQUIRE(a.ldf % 4 == 0 && a.ldd % 4 == 0, "refiner_input: strides must be multiples of 4");
  {
    const int cv = a.dt == DT_F32 ? 4 : 8;
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.feat) | reinterpret_cast<uintptr_t>(a.d)) & 15) == 0;
    const bool vec_off = tuning(SW_RI_VEC) == 0;  // A/B debugging only
    if (!vec_off && aligned && a.C % cv == 0 && a.ldf % cv == 0 && a.ldd % cv == 0) {
      int lpp = 1;
      while (lpp < 64 && lpp * cv < a.C) lpp *= 2;
      const long per_wg = 4 * (64 / lpp);
      dim3 vgrid((unsigned)((npix + per_wg - 1) / per_wg));
      ROMA_DT_SWITCH(a.dt, T, hipLaunchKernelGGL(refiner_input_vec_kernel<T>, vgrid, dim3(256), 0, s, a, lpp));
      ROMA_LAUNCH_CHECK();
      return 0;
    }
  }
  dim3 grid((unsigned)((npix + 3) / 4));
  ROMA_DT_SWITCH(a.dt, T, hipLaunchKernelGGL(refiner_input_kernel<T>, grid, dim3(256), 0, s, a));
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
