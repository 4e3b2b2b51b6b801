// Warp morph rendering (the frames of the reference's demo/demo_3D_effect.py in one enqueue): see morph.hip and
// roma_op_render_morph in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
int render_morph_frame_chunk();
long render_morph_workspace_bytes(int B, int im_h, int im_w, long T);
int render_morph_launch(const float* warp, long warp_batch_stride, long warp_row_stride, const void* image, int image_u8, const double* ts,
                        const float* certainty, long cert_batch_stride, long cert_row_stride, float background, int B, long T, int H, int W,
                        int im_h, int im_w, void* out, int out_f32, void* workspace, long workspace_bytes, hipStream_t s);
}  // namespace roma
