// Scoring tail of the pose and homography benchmarks (the reference's compute_pose_error / pose_auc, romatch/utils/utils.py, the
// accuracy / mAP lines of its pose benchmarks and the corner distance of its HPatches benchmark): see metrics.hip and
// roma_op_pose_error / roma_op_corner_error / roma_op_error_log_append / roma_op_error_summary in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
int pose_error_launch(const double* R, const double* t, const unsigned char* ok, const double* T_gt, int t_rows, int B, double* err,
                      double* log, long capacity, long long* state, hipStream_t s);
int corner_error_launch(const double* H_pred, const unsigned char* ok, const double* H_gt, const double* sizes, int B, double* err,
                        double* log, long capacity, long long* state, hipStream_t s);
int error_log_append_launch(const double* values, int B, double* log, long capacity, long long* state, hipStream_t s);
int error_summary_launch(const double* errors, long n, const long long* state, long capacity, const double* thresholds_host, int T,
                         long long* out_n, long long* out_below, double* out_acc, double* out_auc, hipStream_t s);
}  // namespace roma
