// Cached per-image features: pack layout and the slab gather / scatter kernel (encoded.h).
#include "encoded.h"

#include <algorithm>

#include "arch.h"

namespace roma {

PackLayout pack_layout(int coarse_h, int coarse_w, int upsample_h, int upsample_w, const int* cf, size_t esz) {
  PackLayout L;
  long off = 0;
  for (int ps = 0; ps < 2; ++ps) {
    const int H = ps ? upsample_h : coarse_h, W = ps ? upsample_w : coarse_w;
    for (int si = 0; si < 5; ++si) {
      L.off[ps][si] = -1;
      L.bytes[ps][si] = 0;
      if (H <= 0 || W <= 0 || (ps == 1 && si == 0)) continue;  // the upsample pass has no stride-16 scale
      const int ins = SCALE_INT[si];
      const long hw = ins == 16 ? (long)(H / 14) * (W / 14) : (long)(H / ins) * (W / ins);
      L.off[ps][si] = off;
      L.bytes[ps][si] = hw * round_up(cf[si], 8) * (long)esz;
      off = round_up(off + L.bytes[ps][si], 256);
    }
    if (ps == 0) L.coarse_bytes = off;
  }
  L.total = off;
  return L;
}

// blockIdx.y = slab; the blocks of a row walk the slab's 16-byte units with a grid stride, four units in flight per lane
__global__ __launch_bounds__(256) void slab_copy_kernel(const uint4* __restrict__ src, long src_stride_v, uint4* __restrict__ dst,
                                                        long dst_stride_v, long slab_v, SlabTable t) {
  const int s = blockIdx.y;
  const uint4* __restrict__ ps = src + (long)t.src_idx[s] * src_stride_v;
  uint4* __restrict__ pd = dst + (long)t.dst_idx[s] * dst_stride_v;
  const long step = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * step < slab_v; i += 4 * step) {
    const uint4 a = ps[i], b = ps[i + step], c = ps[i + 2 * step], d = ps[i + 3 * step];
    pd[i] = a;
    pd[i + step] = b;
    pd[i + 2 * step] = c;
    pd[i + 3 * step] = d;
  }
  for (; i < slab_v; i += step) pd[i] = ps[i];
}

static int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

int slab_copy_launch(const void* src, long src_stride, void* dst, long dst_stride, long slab_bytes, const SlabTable& t, hipStream_t st) {
  ROMA_REQUIRE(src && dst && t.n >= 1 && t.n <= SLAB_MAX && slab_bytes > 0, "slab_copy: bad arguments");
  ROMA_REQUIRE(slab_bytes % 16 == 0 && src_stride % 16 == 0 && dst_stride % 16 == 0 &&
                   (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0,
               "slab_copy: slabs, strides and base addresses must be multiples of 16 bytes");
  for (int i = 0; i < t.n; ++i) ROMA_REQUIRE(t.src_idx[i] >= 0 && t.dst_idx[i] >= 0, "slab_copy: negative slab index");
  const long slab_v = slab_bytes / 16;
  // 8 blocks per CU over all slabs; a block's lanes move at least four units each where the slab is that long
  const long want = (slab_v + 1023) / 1024, cap = std::max(1L, (long)device_cus() * 8 / t.n);
  const dim3 grid((unsigned)std::min(want, cap), (unsigned)t.n);
  ProfScope prof("slab_copy", 2.0 * (double)slab_bytes * t.n, "byte", st);
  hipLaunchKernelGGL(slab_copy_kernel, grid, dim3(256), 0, st, static_cast<const uint4*>(src), src_stride / 16, static_cast<uint4*>(dst),
                     dst_stride / 16, slab_v, t);
  ROMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace roma
