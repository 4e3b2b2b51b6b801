// Batched bundle adjustment on the device: cameras and points refined together on the reprojection error by Levenberg-Marquardt
// with the Schur complement - see bundle.hip.
#pragma once
#include "common.h"

namespace roma {
constexpr int ROMA_BA_MAX_VIEWS = 8;   // views of one problem: the reduced camera system is at most 48 x 48
constexpr int BUNDLE_ADJUST_INFO = 6;  // ints per problem in bundle_adjust_launch's out_info

size_t bundle_adjust_workspace_bytes(int B, int V, int N);
// B problems of V views and N points.  points [B, N, 3] f64; kpts [B, V, N, 2] f32, pixels of their view, a non-finite entry: not
// observed; K [B, V, 3, 3] f64 or NULL (kpts are normalised image coordinates, and so is thr); R [B, V, 3, 3], t [B, V, 3] f64
// with x_cam = R X + t; hold [B, V, 6] u8 or NULL (nothing held): camera parameters (three rotation, three translation) that
// stay; counts [B] int32 (NULL: N points each; the kpts of later points are never read, the points themselves are copied
// through); valid [B] u8 (NULL: every problem); thr: the reprojection threshold in pixels of each view's K, +inf: plain least
// squares; at most max_steps accepted steps.
// Outputs: points [B, N, 3], R [B, V, 3, 3], t [B, V, 3] f64 (the input bits without an accepted step, and for every point
// that is not part of the problem), mask [B, V, N] u8 (rows inside the threshold under the state returned; zeros for a problem
// that is not fitted), info [B, BUNDLE_ADJUST_INFO] int32 = {accepted steps, cost evaluations, active rows at the end, points
// adjusted, free camera parameters, problem fitted}, cost [B, 2] f64 = {start, end} (NaN for a problem that is not evaluated).
int bundle_adjust_launch(const double* points, const float* kpts, const double* K, const double* R, const double* t,
                         const unsigned char* hold, const int* counts, const unsigned char* valid, int B, int V, int N, double thr,
                         int max_steps, double* out_points, double* out_r, double* out_t, unsigned char* out_mask, int* out_info,
                         double* out_cost, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
