// Dense multi-view depth fusion: the depth hypotheses the pairs of an image set give every view, fused to one depth map per view
// and one point cloud (depth_fusion.hip).  See roma_op_fuse_depth_maps / roma_op_relative_poses in include/roma_hip.h; restated
// by tools/depth_fusion_ref.py.
#pragma once
#include "common.h"

namespace roma {
constexpr int FUSE_MAX_VIEWS = 8, FUSE_MAX_PAIRS = 64;
constexpr int FUSE_MAX_SLOTS = 2 * (FUSE_MAX_VIEWS - 1);  // hypotheses of one view: (i, j) and (j, i) may both occur
constexpr int FUSE_STATS = 8;                              // ints per problem in fuse_depth_maps_launch's out_stats
constexpr int FUSE_MAX_COLOR_VIEWS = 128;                  // B * V with a colour source: offsets and sizes travel in the kernel's arguments

size_t fuse_depth_maps_workspace_bytes(int B, int V, int H, int W);
int fuse_depth_maps_launch(const float* points, const unsigned char* flags, const float* certainty, const int* pair_views,
                           const double* cameras, const double* R, const double* t, const unsigned char* view_valid,
                           const unsigned char* valid, const unsigned char* images, const long long* image_offsets,
                           const int* image_sizes, int B, int V, int P, int H, int W, int symmetric, double rel_thresh, int min_support,
                           int min_consistent, int max_violations, int dedupe, int max_points, float* out_depth, float* out_weight,
                           unsigned char* out_support, unsigned char* out_seen, unsigned char* out_violated, unsigned char* out_state,
                           float* out_points, unsigned char* out_colors, float* out_cloud_weight, int* out_source, int* out_counts,
                           int* out_total, int* out_stats, void* ws, size_t ws_bytes, hipStream_t s);
int relative_poses_launch(const double* R, const double* t, const int* pair_views, int B, int V, int P, double* out_R, double* out_t,
                          hipStream_t s);
}  // namespace roma
