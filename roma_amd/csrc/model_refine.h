// Batched Levenberg-Marquardt refinement of homographies and fundamental matrices on the truncated reprojection / Sampson
// error - see model_refine.hip.
#pragma once
#include "common.h"

namespace roma {
constexpr int REFINE_MODEL_INFO = 4;  // ints per pair in out_info
constexpr int REFINE_MODEL_COST = 2;  // doubles per pair in out_cost
size_t refine_model_workspace_bytes(int B, int N);
// model: RANSAC_HOMOGRAPHY (0) or RANSAC_FUNDAMENTAL (1).  M [B, 3, 3] f64: the models to refine, in pixel coordinates
// (x_B ~ H x_A, x_B^T F x_A = 0); kpts_a / kpts_b [B, N, 2] f32 pixels; counts [B] int32 (NULL: N rows each); valid [B] u8 (NULL:
// every pair): pairs to fit, the others are copied through; thr: the truncation threshold in pixels (inf: plain least
// squares); at most max_steps accepted steps.  Outputs: M [B, 3, 3] f64 (scaled like roma_op_ransac's after an accepted
// step, else the input), mask [B, N] u8 (residual below thr under the returned model; zeros for a pair that is not fitted),
// info [B, REFINE_MODEL_INFO] int32 = {accepted steps, cost evaluations, active rows at the end, pair fitted}, cost
// [B, REFINE_MODEL_COST] f64 = {truncated cost at the start, at the end} in px^2 (NaN for a pair that is not fitted).  Every
// pointer is device memory; nothing is read back.
int refine_model_launch(int model, const double* M, const float* kpts_a, const float* kpts_b, const int* counts,
                        const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_m, unsigned char* out_mask,
                        int* out_info, double* out_cost, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
