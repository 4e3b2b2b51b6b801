// Ground-truth warp from sensor depth (the reference's warp_kpts / get_gt_warp) and the dense EPE / PCK metrics built on it
// (MegadepthDenseBenchmark.geometric_dist): see gt_warp.hip and roma_op_warp_kpts / roma_op_dense_metrics in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
int warp_kpts_launch(const void* kpts, int kpts_f64, int grid_h, int grid_w, const float* depth0, const float* depth1, const double* T,
                     int t_rows, const double* K0, const double* K1, int B, long L, int H0, int W0, int H1, int W1, double rel_thresh,
                     unsigned char* valid, float* prob, double* rel, double* warped, hipStream_t s);
long dense_metrics_workspace_bytes(int B, int h, int w);
int dense_metrics_launch(const float* matches, long batch_stride, long row_stride, const float* depth1, const float* depth2,
                         const double* T, int t_rows, const double* K1, const double* K2, int B, int h, int w, int H1, int W1, int H2,
                         int W2, double rel_thresh, double thr0, double thr1, double thr2, long long* n_valid, long long* n_below,
                         double* gd_sum, double* epe, double* pck, float* prob, double* gd, void* workspace, long workspace_bytes,
                         hipStream_t s);
}  // namespace roma
