// Batched Levenberg-Marquardt refinement of a relative pose on the Sampson error (truncated loss) - see pose_refine.hip.
#pragma once
#include "common.h"

namespace roma {
constexpr int REFINE_POSE_INFO = 4;  // ints per pair in out_info
size_t refine_pose_workspace_bytes(int B, int N);
// R [B, 3, 3], t [B, 3] f64: the poses to refine; kpts_a / kpts_b [B, N, 2] f32 NORMALISED points (x_b^T [t]x R x_a = 0); counts
// [B] int32 (NULL: N rows each); valid [B] u8 (NULL: every pair): pairs to fit, the others are copied through; thr: the
// truncation threshold in normalised units; at most max_steps accepted steps.  Outputs: R [B, 3, 3], t [B, 3] f64 (unit norm
// after an accepted step, else the input), mask [B, N] u8 (Sampson error below thr and in front of both cameras; zeros for a pair
// that is not fitted), info [B, REFINE_POSE_INFO] int32 = {accepted steps, cost evaluations, active rows at the end, pair
// fitted (valid, at least 5 rows, finite pose)}.  Every pointer is device memory; nothing is read back.
int refine_pose_launch(const double* R, const double* t, const float* kpts_a, const float* kpts_b, const int* counts,
                       const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_r, double* out_t,
                       unsigned char* out_mask, int* out_info, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
