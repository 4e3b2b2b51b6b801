// RegressionMatcher.match_keypoints (romatch/models/matcher.py:732-773) for every pair of a batch in one enqueue of five launches,
// nothing read back, nothing allocated: see keypoints_batched.hip and roma_op_match_keypoints in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
long match_keypoints_workspace_bytes(int B, long NA, long NB);
int match_keypoints_launch(const float* x_a, const float* x_b, const int* counts_a, const int* counts_b, const float* warp,
                           long warp_batch_stride, long warp_row_stride, const float* certainty, long cert_batch_stride,
                           long cert_row_stride, const float* sizes, long sizes_batch_stride, int B, long NA, long NB, int H, int W,
                           float max_dist, float cert_th, long M, int* inds, float* kpts_a, float* kpts_b, int* counts,
                           long long* total, void* workspace, long workspace_bytes, hipStream_t s);
}  // namespace roma
