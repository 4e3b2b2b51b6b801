// Point-cloud rendering: N world points splatted into C cameras with a z-buffer of packed 64-bit keys, then an occlusion filter and
// a hole fill (point_render.hip).  See roma_op_render_points in include/roma_hip.h; restated by tools/point_render_ref.py.
#pragma once
#include "common.h"

namespace roma {
constexpr int RENDER_MAX_RADIUS = 4;  // splat, occlusion and fill windows: at most 9 x 9
constexpr int RENDER_STATS = 4;       // ints per frame in render_points_launch's out_stats

size_t render_points_workspace_bytes(int B, int C, int H, int W);
int render_points_launch(const float* points, const unsigned char* colors, const int* counts, const unsigned char* valid,
                         const double* cameras, const double* R, const double* t, int B, int N, int C, int H, int W, int radius,
                         double near, double far, int occlusion_radius, double occlusion_rel, int occlusion_count, int fill_radius,
                         int fill_min, int background, unsigned char* out_color, float* out_depth, int* out_index,
                         unsigned char* out_mask, int* out_stats, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
