// Batched RANSAC on the device: homography (4-point DLT) and fundamental matrix (7-point) - see geometry.hip and ransac.h.
#pragma once
#include "common.h"

namespace roma {
constexpr int RANSAC_HOMOGRAPHY = 0, RANSAC_FUNDAMENTAL = 1;
constexpr int RANSAC_INFO = 6;         // ints per pair in out_info
size_t ransac_workspace_bytes(int B, int N);
// kpts_a / kpts_b [B, N, 2] f32 pixels; counts [B] int32 (NULL: N rows each); seeds [B] u64.  Outputs: model [B, 3, 3] f64,
// mask [B, N] u8, ok [B] u8, info [B, RANSAC_INFO] int32 = {rounds, winning hypothesis, its root, its inlier count, final
// inlier count, pair valid}.  Every pointer is device memory; nothing is read back.
int ransac_launch(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B,
                  int N, float threshold, double confidence, int max_iters, int refine, double* out_model, unsigned char* out_mask,
                  unsigned char* out_ok, int* out_info, void* ws, size_t ws_bytes, hipStream_t s);

// The same RANSAC with MAGSAC++ scoring and IRLS local optimisation (ransac.h, tools/magsac_ref.py).  Inputs as for
// ransac_launch; lo_iters in [0, MAGSAC_MAX_LO].  info [B, MAGSAC_INFO] = the RANSAC_INFO entries (inlier counts: r < threshold)
// and the LO steps accepted; score f64 [B, 2] = {sum of rho of the winning minimal model, final sum: that less the LO gains}
// (0 without a model).
constexpr int MAGSAC_INFO = RANSAC_INFO + 1;
constexpr int MAGSAC_MAX_LO = 64;
size_t magsac_workspace_bytes(int B, int N);
int magsac_launch(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B,
                  int N, float threshold, double confidence, int max_iters, int lo_iters, double* out_model, unsigned char* out_mask,
                  unsigned char* out_ok, int* out_info, double* out_score, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
