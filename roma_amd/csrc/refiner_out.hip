// ConvRefiner out_conv (C -> 3, f32) + flow / certainty update, and the FINAL refiner blocks' delta pass (see elementwise.h).
#include <algorithm>
#include "elementwise_device.h"
#include "tuning.h"

namespace roma {

template <typename T, int G>
__global__ __launch_bounds__(256) void refiner_out_kernel(const T* d, long ldd, const float* w, const float* bb, float* flow,
                                                          float* cert, long M, int Cp, float sx, float sy) {
  const int lane = threadIdx.x & 63;
  const int sub = lane % G, rw = lane / G;
  constexpr int RPW = 64 / G;
  const long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + rw;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  if (row < M) {
    for (int c = sub * 4; c < Cp; c += G * 4) {
      const f32x4 v = ElemIO<T>::ld4(d + row * ldd + c);
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + c);
      const f32x4 w1 = *reinterpret_cast<const f32x4*>(w + Cp + c);
      const f32x4 w2 = *reinterpret_cast<const f32x4*>(w + 2 * Cp + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a0 = fmaf(v[j], w0[j], a0);
        a1 = fmaf(v[j], w1[j], a1);
        a2 = fmaf(v[j], w2[j], a2);
      }
    }
  }
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) {
    a0 += __shfl_xor(a0, off);
    a1 += __shfl_xor(a1, off);
    a2 += __shfl_xor(a2, off);
  }
  if (row < M && sub == 0) {
    flow[row * 2 + 0] += sx * (a0 + bb[0]);
    flow[row * 2 + 1] += sy * (a1 + bb[1]);
    cert[row] += a2 + bb[2];
  }
}

// Vectorised form: LPR lanes (a power of two) share a row, 16 bytes per lane per access, and a wave walks ROWS_IT
// groups of 64/LPR rows with its out_conv weights held in registers.  (The kernel above re-read 48 bytes of f32
// weights from L1/L2 for every 8 bytes of activations and left 28 of 64 lanes idle at Cp = 144: 4x off the HBM bound.)
template <typename T, int NK>
__global__ __launch_bounds__(256) void refiner_out_vec_kernel(const T* d, long ldd, const float* w, const float* bb,
                                                              float* flow, float* cert, long M, int Cp, float sx, float sy,
                                                              int lpr, int rows_it) {
  constexpr int CV = VecIO<T>::CV;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (lpr - 1), rw = lane / lpr, rpw = 64 / lpr;
  // the lane's 3 x NK x CV out_conv weights, fetched as 16-byte pieces with a clamped index and selected afterwards (Cp is a
  // multiple of CV, refiner_out_launch checks w's alignment).  As 120 guarded 4-byte loads - a branch around each - this
  // prologue took a third of a workgroup's life at Cp = 576 (round 6, late: tools/bench_refiner_out.py).
  float wr[NK][3][CV];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int c = (sub + k * lpr) * CV;
    const bool okc = c < Cp;
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
      for (int j4 = 0; j4 < CV; j4 += 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(w + (long)o * Cp + (okc ? c : 0) + j4);
#pragma unroll
        for (int u = 0; u < 4; ++u) wr[k][o][j4 + u] = okc ? t[u] : 0.f;
      }
  }
  const float b0 = bb[0], b1 = bb[1], b2 = bb[2];
  const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw * rows_it + rw;
  // Round 6 (late): the row groups are software-pipelined - the 16-byte pieces (and flow / certainty) of group it + 1 are
  // requested BEFORE the ~240 VALU instructions and the shuffle reduction of group it, into a second register set (the loop
  // runs in pairs, so the two sets swap roles without moves).  The `#pragma unroll 4` this replaces never happened (rows_it
  // is a run-time value): a wave had 5 x 16 bytes per lane in flight, waited, computed with nothing in flight - 1.9 TB/s
  // at Cp = 576 / 1152 (profiles/r06_final_bench_mixed_kernel_stats.csv of commit 49f591d: 0.98 ms per step for 1.83 GB).
  // Same loads, same arithmetic in the same order: bit-identical.
  typedef typename VecIO<T>::Raw Raw;
  struct Group {
    Raw v[NK];
    float f0, f1, c0;
  };
  auto fetch = [&](Group& g, long row) __attribute__((always_inline)) {
    // branch-free loads (clamped row and chunk, select afterwards): inside exec-masked blocks hipcc waits for every load on
    // its own, and this kernel is nothing but loads (1.5 TB/s at Cp = 144 with the guarded form)
    const long rowc = row < M ? row : M - 1;
    // the running flow / certainty are fetched with the activations, not after the reduction (a dependent
    // load -> add -> store tail per row group otherwise)
    g.f0 = flow[rowc * 2 + 0];
    g.f1 = flow[rowc * 2 + 1];
    g.c0 = cert[rowc];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int c = (sub + k * lpr) * CV;
      g.v[k] = VecIO<T>::ldraw(d + rowc * ldd + (c < Cp ? c : 0));
    }
  };
  auto finish = [&](const Group& g, long row) __attribute__((always_inline)) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      float v[CV];
      VecIO<T>::cvt(g.v[k], v);
      const bool ok = (sub + k * lpr) * CV < Cp;
#pragma unroll
      for (int j = 0; j < CV; ++j) {
        const float x = ok ? v[j] : 0.f;
        a0 = fmaf(x, wr[k][0][j], a0);
        a1 = fmaf(x, wr[k][1][j], a1);
        a2 = fmaf(x, wr[k][2][j], a2);
      }
    }
    for (int off = lpr >> 1; off >= 1; off >>= 1) {
      a0 += __shfl_xor(a0, off);
      a1 += __shfl_xor(a1, off);
      a2 += __shfl_xor(a2, off);
    }
    if (row < M && sub == 0) {
      flow[row * 2 + 0] = g.f0 + sx * (a0 + b0);
      flow[row * 2 + 1] = g.f1 + sy * (a1 + b1);
      cert[row] = g.c0 + (a2 + b2);
    }
  };
  Group ga, gb;
  fetch(ga, row0);
  for (int it = 0; it < rows_it; it += 2) {  // rows_it is even (refiner_out_launch)
    const long row = row0 + (long)it * rpw;
    fetch(gb, row + rpw);
    finish(ga, row);
    if (it + 2 < rows_it) fetch(ga, row + 2 * rpw);  // uniform
    finish(gb, row + rpw);
  }
}

// Narrow rows (bf16, Cp = 24: the stride-1 refiner, 12 M pixels per call): ONE LANE PER ROW.  The shared-row kernel above
// gives such a row to two lanes (3 chunks: the second lane idles in the second piece, 2.8 TB/s); here a lane reads its
// row's NCH 16-byte chunks itself (the 48-byte lane stride leaves every fetched line fully used across the NCH loads,
// L1 serves the repeats), keeps all 3 x Cp weights in registers over ROWS rows, needs no shuffles, and the running
// flow / certainty are lane-contiguous 8- and 4-byte accesses.
template <int NCH, int ROWS>
__global__ __launch_bounds__(256) void refiner_out_row_kernel(const bf16_t* d, long ldd, const float* w, const float* bb,
                                                              float* flow, float* cert, long M, int Cp, float sx, float sy) {
  float wr[3][NCH * 8];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int j = 0; j < NCH * 8; ++j) wr[o][j] = j < Cp ? w[(long)o * Cp + j] : 0.f;
  const float b0 = bb[0], b1 = bb[1], b2 = bb[2];
  const long row0 = (long)blockIdx.x * 256 * ROWS + threadIdx.x;
#pragma unroll 2
  for (int it = 0; it < ROWS; ++it) {
    const long row = row0 + (long)it * 256;
    if (row >= M) break;
    const f32x2 f = *reinterpret_cast<const f32x2*>(flow + row * 2);
    const float c0 = cert[row];
    float v[NCH][8];
#pragma unroll
    for (int k = 0; k < NCH; ++k) VecIO<bf16_t>::ld(d + row * ldd + k * 8, v[k]);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a0 = fmaf(v[k][j], wr[0][k * 8 + j], a0);
        a1 = fmaf(v[k][j], wr[1][k * 8 + j], a1);
        a2 = fmaf(v[k][j], wr[2][k * 8 + j], a2);
      }
    *reinterpret_cast<f32x2*>(flow + row * 2) = f32x2{f[0] + sx * (a0 + b0), f[1] + sy * (a1 + b1)};
    cert[row] = c0 + (a2 + b2);
  }
}

// flow / certainty += the per-pixel deltas the FINAL refiner blocks wrote (refiner_block.h): flow [M][2], cert [M], delta [M][4]
__global__ __launch_bounds__(256) void refiner_apply_delta_kernel(const f32x4* __restrict__ delta, float* __restrict__ flow,
                                                                  float* __restrict__ cert, long M, float sx, float sy) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long)gridDim.x * 256) {
    const f32x4 d = delta[i];
    f32x2 f = *reinterpret_cast<const f32x2*>(flow + 2 * i);
    f[0] += sx * d[0];
    f[1] += sy * d[1];
    *reinterpret_cast<f32x2*>(flow + 2 * i) = f;
    cert[i] += d[2];
  }
}

int refiner_apply_delta_launch(const float* delta, float* flow, float* cert, long M, float sx, float sy, hipStream_t s) {
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(delta) & 15) == 0 && (reinterpret_cast<uintptr_t>(flow) & 7) == 0, "refiner_apply_delta: alignment");
  const long nb = std::min<long>((M + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(refiner_apply_delta_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const f32x4*)delta, flow, cert, M, sx, sy);
  ROMA_LAUNCH_CHECK();
  return 0;
}

int refiner_out_launch(const void* d, long ldd, int dt, const float* w, const float* b, float* flow, float* cert,
                       long M, int Cp, float sx, float sy, hipStream_t s) {
  ROMA_REQUIRE(Cp % 4 == 0 && ldd % 4 == 0, "refiner_out: channel padding must be a multiple of 4");
  const int row_env = tuning(SW_OUT_ROW);
  if (row_env && dt == DT_BF16 && Cp == 24 && ldd % 8 == 0 && (reinterpret_cast<uintptr_t>(d) & 15) == 0 &&
      (reinterpret_cast<uintptr_t>(flow) & 7) == 0) {
    constexpr int ROWS = 8;
    dim3 grid((unsigned)((M + 256l * ROWS - 1) / (256l * ROWS)));
    hipLaunchKernelGGL((refiner_out_row_kernel<3, ROWS>), grid, dim3(256), 0, s, (const bf16_t*)d, ldd, w, b, flow, cert, M, Cp, sx, sy);
    ROMA_LAUNCH_CHECK();
    return 0;
  }
  {
    const int cv = dt == DT_F32 ? 4 : 8;
    const int chunks = Cp / cv;
    if (Cp % cv == 0 && ldd % cv == 0 && (reinterpret_cast<uintptr_t>(d) & 15) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0 && chunks >= 1) {
      int lpr = 1;
      while (lpr < 64 && lpr * 2 <= chunks) lpr *= 2;       // largest power of two <= chunks (<= 64)
      // bf16: chunk counts just above a power of two (18, 72, 144) leave 44 % of the lane-pieces of that split empty (the
      // second piece has 2 / 8 / 16 active lanes of 16 / 64 / 64): take the power of two that fills the pieces best with
      // at most 5 per lane (18 = 4 x 5 - 2, 72 = 16 x 5 - 8, 144 = 32 x 5 - 16: 90 %), which also shortens the shuffle
      // reduction.  The f32 mode keeps its split (bit-for-bit history of the parity runs).
      const int lpr_env = tuning(SW_OUT_LPR);
      if (dt == DT_BF16 && lpr_env) {
        int best_l = lpr;
        double best_e = (double)chunks / ((double)lpr * ((chunks + lpr - 1) / lpr));
        for (int l = lpr / 2; l >= 2; l /= 2) {
          const int n = (chunks + l - 1) / l;
          if (n > 5) break;
          const double e = (double)chunks / ((double)l * n);
          if (e > best_e + 1e-9) {
            best_e = e;
            best_l = l;
          }
        }
        lpr = best_l;
      }
      const int nk = (chunks + lpr - 1) / lpr;              // 16-byte pieces per lane per row
      if (nk <= 6) {
        // 8 row groups per wave.  (With the weight prologue as guarded scalar loads 32 groups were 1.5 x faster than 8; with the
        // 16-byte prologue 8 and 16 are equal and 32 loses on the sub-batch sizes - profiles/r06_v39_*.  ROMA_OUT_ROWS_IT: A/B, even.)
        const int rows_it_env = tuning(SW_OUT_ROWS_IT);
        const int rows_it = rows_it_env >= 2 ? rows_it_env & ~1 : 8;
        const long rows_per_block = 4l * (64 / lpr) * rows_it;
        dim3 grid((unsigned)((M + rows_per_block - 1) / rows_per_block));
#define ROMA_ROV(NKV)                                                                                          \
  ROMA_DT_SWITCH(dt, T, hipLaunchKernelGGL((refiner_out_vec_kernel<T, NKV>), grid, dim3(256), 0, s, (const T*)d, ldd, w, b, \
                                           flow, cert, M, Cp, sx, sy, lpr, rows_it))
        if (nk <= 1) { ROMA_ROV(1); }
        else if (nk == 2) { ROMA_ROV(2); }
        else if (nk == 3) { ROMA_ROV(3); }
        else if (nk == 5) { ROMA_ROV(5); }
        else { ROMA_ROV(6); }
#undef ROMA_ROV
        ROMA_LAUNCH_CHECK();
        return 0;
      }
    }
  }
  const int chunks = Cp / 4;
#define ROMA_RO(G)                                                                                          \
  {                                                                                                         \
    const long rows_per_block = 4 * (64 / G);                                                               \
    dim3 grid((unsigned)((M + rows_per_block - 1) / rows_per_block));                                       \
    ROMA_DT_SWITCH(dt, T, hipLaunchKernelGGL((refiner_out_kernel<T, G>), grid, dim3(256), 0, s, (const T*)d, ldd, w, b, \
                                             flow, cert, M, Cp, sx, sy));                                   \
  }
  if (chunks <= 8) ROMA_RO(8)
  else if (chunks <= 16) ROMA_RO(16)
  else if (chunks <= 32) ROMA_RO(32)
  else ROMA_RO(64)
#undef ROMA_RO
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
