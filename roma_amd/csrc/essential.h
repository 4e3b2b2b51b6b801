// Batched essential-matrix RANSAC (five-point solver) and recoverPose on the device - see essential.hip and ransac.h.
#pragma once
#include "common.h"

namespace roma {
constexpr int ESSENTIAL_MAX_ROOTS = 10;  // real solutions of one five-point sample (tools/essential_ref.py: MAX_ROOTS)
constexpr int ESSENTIAL_INFO = 5;        // ints per pair in out_info
size_t essential_workspace_bytes(int B, int N);
// kpts_a / kpts_b [B, N, 2] f32; counts [B] int32 (NULL: N rows each); seeds [B] u64; K [B, 3, 3] f64 camera matrix (NULL:
// identity, the points are normalised already).  Outputs: E [B, 3, 3] f64 (unit Frobenius norm, largest-magnitude entry
// positive), mask [B, N] u8, ok [B] u8, info [B, ESSENTIAL_INFO] int32 = {rounds, winning hypothesis, its root, inlier count,
// pair valid}.  Every pointer is device memory; nothing is read back.
int essential_launch(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, const double* K,
                     int B, int N, float threshold, double prob, int max_iters, double* out_e, unsigned char* out_mask,
                     unsigned char* out_ok, int* out_info, void* ws, size_t ws_bytes, hipStream_t s);
// The same sampling with MAGSAC++ scoring and local optimisation (ransac.h MagsacScoring, tools/essential_magsac_ref.py): a model's
// score is the sum of the MAGSAC++ loss of its Sampson distance in normalised camera coordinates, then up to lo_iters (0 ..
// ESSENTIAL_MAGSAC_MAX_LO) IRLS steps, each kept only if the score drops.  Inputs as for essential_launch.  info
// [B, ESSENTIAL_MAGSAC_INFO] = {rounds, winning hypothesis, its root, inliers of the winning minimal model, final inliers, pair
// valid, LO steps accepted}; score f64 [B, 2] = {sum of rho of the winning minimal model, final sum} (0 without a model).
constexpr int ESSENTIAL_MAGSAC_INFO = 7;
constexpr int ESSENTIAL_MAGSAC_MAX_LO = 64;
size_t essential_magsac_workspace_bytes(int B, int N);
int essential_magsac_launch(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                            const double* K, int B, int N, float threshold, double prob, int max_iters, int lo_iters, double* out_e,
                            unsigned char* out_mask, unsigned char* out_ok, int* out_info, double* out_score, void* ws,
                            size_t ws_bytes, hipStream_t s);
// the five-point solver alone: x0, x1 [S, 5, 2] f64 (x1^T E x0 = 0) -> E [S, ESSENTIAL_MAX_ROOTS, 3, 3] f64 (unused slots 0),
// n [S] int32 real solutions in ascending order of Nister's z
int essential_minimal_launch(const double* x0, const double* x1, int S, double* out_e, int* out_n, hipStream_t s);
size_t recover_pose_workspace_bytes(int B, int N);
// cv2.recoverPose: E [B, 3, 3] f64; kpts [B, N, 2] f32; mask [B, N] u8 (NULL: every row); counts, K as above.  Outputs:
// n_good [B] int32, R [B, 3, 3] f64, t [B, 3] f64, mask_good [B, N] u8.
int recover_pose_launch(const double* E, const float* kpts_a, const float* kpts_b, const unsigned char* mask, const int* counts,
                        const double* K, int B, int N, double distance_thresh, int* out_n, double* out_r, double* out_t,
                        unsigned char* out_mask, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
