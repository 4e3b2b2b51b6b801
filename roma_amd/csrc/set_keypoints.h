// Detector-free keypoints (set_keypoints.hip): the dense matches sample_batched draws for the pairs of V <= 8 images, quantised
// to one keypoint per occupied pixel cell of every view and re-indexed to those keypoints - what build_tracks reads.
// See roma_op_keypoints_from_matches in include/roma_hip.h; restated by tools/set_keypoints_ref.py.
#pragma once
#include "tracks.h"

namespace roma {
constexpr int SET_KPTS_INFO = 6;              // ints per problem in keypoints_from_matches_launch's out_info
constexpr int SET_KPTS_MAX_CELL = 64;         // pixels
constexpr int SET_KPTS_MAX_SIZE = 65535;      // H and W of a view
constexpr long SET_KPTS_MAX_GRID = 1l << 22;  // cells of one view
constexpr long SET_KPTS_MAX_CELLS = 1l << 28; // B (G_total + 1024 V): the cells of a call with every view's grid padded to a block

size_t keypoints_from_matches_workspace_bytes(int B, int V, int P, int N, long G_total, int K);
// pair_views [P, 2] and sizes [V, 2] = (H, W) are HOST memory: checked before any device work and passed by value.  Everything
// else as in include/roma_hip.h.
int keypoints_from_matches_launch(const float* matches, const float* certainty, const int* counts, const int* pair_views,
                                  const int* sizes, int B, int V, int P, int N, int cell, float radius, int K, int one_to_one,
                                  float* out_kpts, float* out_score, int* out_num_kpts, int* out_total, int* out_inds, int* out_kept,
                                  int* out_info, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
