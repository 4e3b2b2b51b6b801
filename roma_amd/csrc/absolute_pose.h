// Batched absolute pose on the device: P3P RANSAC, Levenberg-Marquardt refinement of the reprojection error, and the lifting
// of matches to 3-D points through a depth map - see absolute_pose.hip.
#pragma once
#include "common.h"

namespace roma {
constexpr int ABSOLUTE_POSE_INFO = 5;         // ints per pair in absolute_pose_launch's out_info
constexpr int ABSOLUTE_POSE_SLOTS = 4;        // solutions of one P3P sample
constexpr int REFINE_ABSOLUTE_POSE_INFO = 4;  // ints per pair in refine_absolute_pose_launch's out_info

size_t absolute_pose_workspace_bytes(int B, int N);
// points3d [B, N, 3], kpts [B, N, 2] f32: rows (X, x) with x ~ K (R X + t); counts [B] int32 (NULL: N rows each; later rows are
// never read); seeds [B] u64; K [B, 3, 3] f64 or NULL (kpts are normalised image coordinates); thr: the reprojection threshold
// in pixels of K (in normalised units without K).  Outputs: R [B, 3, 3], t [B, 3] f64 (zero without a model), mask [B, N] u8, ok
// [B] u8, info [B, ABSOLUTE_POSE_INFO] int32 = {rounds, winning hypothesis, its slot, its inlier count, pair valid}.
int absolute_pose_launch(const float* points3d, const float* kpts, const int* counts, const unsigned long long* seeds, const double* K,
                         int B, int N, float thr, double conf, int max_iters, double* out_r, double* out_t, unsigned char* out_mask,
                         unsigned char* out_ok, int* out_info, void* ws, size_t ws_bytes, hipStream_t s);
// the P3P solver alone: X [S, 3, 3] f64 points, x [S, 3, 2] f64 normalised image points -> R [S, 4, 3, 3], t [S, 4, 3] f64 (unused
// slots zero), n [S] int32 solutions per sample, ascending in the solver's root
int absolute_pose_minimal_launch(const double* X, const double* x, int S, double* out_r, double* out_t, int* out_n, hipStream_t s);
// R [B, 3, 3], t [B, 3] f64: the poses to refine on the rows of absolute_pose_launch; valid [B] u8 (NULL: every pair): pairs to
// fit, the others are copied through; at most max_steps accepted steps.  Outputs: R, t (the input without an accepted step), mask
// [B, N] u8 (positive depth and reprojection error below thr; zeros for a pair that is not fitted), info
// [B, REFINE_ABSOLUTE_POSE_INFO] int32 = {accepted steps, cost evaluations, active rows at the end, pair fitted}.
int refine_absolute_pose_launch(const double* R, const double* t, const float* points3d, const float* kpts, const int* counts,
                                const unsigned char* valid, const double* K, int B, int N, double thr, int max_steps, double* out_r,
                                double* out_t, unsigned char* out_mask, int* out_info, hipStream_t s);
// matches [B, N, 4] f32 in normalised coordinates (columns 0:2 in A, 2:4 in B), depth [B, H, W] f32 of image A, K [B, 3, 3] f64
// of image A at the depth map's size -> points [B, N, 3] f32 in camera A's frame (NaN where one of the four bilinear neighbours
// is outside, not finite or not positive), kpts_b [B, N, 2] f32 pixels of an image of (H_B, W_B)
int lift_matches_launch(const float* matches, const float* depth, const double* K, int B, int N, int H, int W, int H_B, int W_B,
                        float* out_points, float* out_kpts, hipStream_t s);
}  // namespace roma
