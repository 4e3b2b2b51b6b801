// Cached per-image features (roma_encode / roma_match_encoded): the layout of one image's feature pack and the slab copy
// that moves projected feature maps between the schedule's contiguous buffers and the packs.
#pragma once
#include "common.h"

namespace roma {

// One image's pack: for each pass (coarse, then upsample when the handle has one) and each scale of the pass (16 | 8, 4, 2, 1)
// the projected map [hw, ldf] in the activation type, ldf = round_up(PROJ_COUT, 8); every segment starts on a 256-byte boundary
// and so does the next image's pack.  Pure host arithmetic (roma_amd/encoded.py::pack_layout restates it).
struct PackLayout {
  long off[2][5] = {{0}};    // byte offset of segment [pass][scale index]; -1: the pass has no such scale
  long bytes[2][5] = {{0}};  // hw * ldf * esz (a multiple of 16)
  long total = 0;            // bytes of one pack
  long coarse_bytes = 0;     // ... of its coarse part (what roma_encode fills without high-resolution images)
};
PackLayout pack_layout(int coarse_h, int coarse_w, int upsample_h, int upsample_w, const int* cf, size_t esz);

// n <= SLAB_MAX slabs of slab_bytes each: slab i goes from src + src_idx[i] * src_stride to dst + dst_idx[i] * dst_stride
// (bytes, 64-bit).  The indices travel in the kernel's argument block: they are host values, checked by the caller.
constexpr int SLAB_MAX = 32;
struct SlabTable {
  int n = 0;
  int src_idx[SLAB_MAX] = {0};
  int dst_idx[SLAB_MAX] = {0};
};
// slab_bytes, both strides and both base addresses must be multiples of 16
int slab_copy_launch(const void* src, long src_stride, void* dst, long dst_stride, long slab_bytes, const SlabTable& t, hipStream_t st);

}  // namespace roma
