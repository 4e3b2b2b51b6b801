/* libroma_hip - the registration operators of the C ABI: similarity (or rigid) transforms between sets of corresponding 3-D
 * points, y ~ s R x + t.  What joins two reconstructions that share views, and what a recovered trajectory or cloud is scored
 * against ground truth with.  Defined in roma_amd/csrc/registration.hip, restated in numpy float64 by tools/registration_ref.py.
 *
 * The declarations sit here, not in roma_hip.h: that header is the table of ROMA_ABI_VERSION, pinned entry by entry, and an
 * operator family that no existing caller needs extends the library without rewriting it.  Both libraries export every name
 * below; roma_amd/_lib.py binds them from this file (EXTENSIONS) exactly as it binds roma_hip.h.
 *
 * Conventions as in roma_hip.h: DEVICE pointers unless stated otherwise; `stream` is a hipStream_t passed as void* (NULL = default
 * stream); calls are asynchronous on that stream; return 0 on success, negative on error (text: roma_last_error()).  Every
 * argument is checked before anything is enqueued.  R is row-major; x_cam = R X + t for cameras.
 */
#ifndef ROMA_HIP_REGISTRATION_H
#define ROMA_HIP_REGISTRATION_H
#ifdef __cplusplus
extern "C" {
#endif

/* Robust similarity between rows of corresponding points: three-point RANSAC through the pipeline of roma_op_ransac (rounds of
 * 256 hypotheses, counter-based samples from (seed, hypothesis), OpenCV's adaptive iteration count, no host synchronisation).
 * src, dst DEVICE f32 [B, N, 3]; counts DEVICE int32 [B] or NULL (N rows each; later rows are never read); seeds DEVICE u64 [B].
 * A hypothesis is the closed form on its three rows: Horn's quaternion for R (always a proper rotation), Umeyama's scale
 * s = sum y'.R x' / sum |x'|^2 (1 when with_scale = 0), t = yb - s R xb; no model for a sample collinear in either set
 * (|d12 x d13| < 1e-4 |d12| |d13|).  Inlier: |s R x + t - y| < threshold, a distance in dst's units.  Both sets are centred and
 * scaled to mean distance 1 first (with_scale = 0: both by src's scale), so the f32 scoring is independent of origin and unit.
 * A row with a non-finite entry is never sampled and never an inlier.  A model needs 4 inliers.  Outputs: scale f64 [B], R f64
 * [B, 3, 3], t f64 [B, 3] (0 where no model), mask u8 [B, N], ok u8 [B], info int32 [B, 5] = {rounds run, winning hypothesis,
 * its slot (0), its inlier count, problem valid (at least 4 finite rows, neither set one point)}.  Bit-identical from run to run
 * and independent of B.  workspace: device memory of roma_op_align_points_workspace(B, N) bytes. */
long roma_op_align_points_workspace(int B, int N);
int roma_op_align_points(const float* src, const float* dst, const int* counts, const unsigned long long* seeds, int B, int N,
                         float threshold, double conf, int max_iters, int with_scale, double* out_scale, double* out_r, double* out_t,
                         unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* workspace, long workspace_bytes,
                         void* stream);
/* The closed form alone on caller-chosen samples: X, Y DEVICE f64 [S, 3, 3] (three points each) -> scale f64 [S], R f64 [S, 3, 3],
 * t f64 [S, 3], n int32 [S] (1: a model; 0: none, and zeros). */
int roma_op_similarity_minimal(const double* X, const double* Y, int S, int with_scale, double* out_scale, double* out_r,
                               double* out_t, int* out_n, void* stream);
/* Refinement under the truncated loss sum min(|r|^2, thr^2) over the finite rows, r = s R x + t - y: a step is the closed form on
 * the rows with |r| < thr under the current model, kept only if the loss is strictly lower; otherwise the loop stops (at most
 * max_steps steps).  scale f64 [B], R f64 [B, 3, 3], t f64 [B, 3]: the start, or all three NULL - no start, the first step fits
 * every finite row.  thr = +inf: no truncation (one step is plain Umeyama).  valid DEVICE u8 [B] or NULL (every problem): the
 * problems to fit.  Outputs: scale, R, t (the input bits - zeros without a start - when no step was accepted), mask u8 [B, N]
 * (the rows with |r| < thr under the returned model), info int32 [B, 4] = {accepted steps, loss evaluations, active rows,
 * problem fitted (valid, at least 3 finite rows, a finite start)}, cost f64 [B, 2] = {loss at the start (+inf without one), at
 * the end} in dst's squared units.  One workgroup per problem; bit-identical from run to run and independent of B. */
int roma_op_refine_similarity(const double* scale, const double* R, const double* t, const float* src, const float* dst,
                              const int* counts, const unsigned char* valid, int B, int N, double thr, int max_steps,
                              int with_scale, double* out_scale, double* out_r, double* out_t, unsigned char* out_mask,
                              int* out_info, double* out_cost, void* stream);
/* X' = s R X + t on points f32 [B, N, 3] (f64 arithmetic, rounded once; NaN stays NaN), and on cameras cam_R f64 [B, V, 3, 3],
 * cam_t f64 [B, V, 3]: R_c' = R_c R^T, t_c' = s t_c - R_c' t - the cameras see the moved points as before, the scene scaled by s.
 * Either half may be absent: its pointers NULL and its N or V equal to 0. */
int roma_op_apply_similarity(const double* scale, const double* R, const double* t, const float* points, int N,
                             const double* cam_R, const double* cam_t, int V, int B, float* out_points, double* out_cam_R,
                             double* out_cam_t, void* stream);
/* Rows of one image that two reconstructions a and b share: every step-th pixel in each direction (row-major,
 * N = ceil(H / step) ceil(W / step)) back-projected at its centre (u + 0.5, v + 0.5) through depth_b and pose b into b's world
 * (src) and through depth_a and pose a into a's world (dst).  depth_a, depth_b DEVICE f32 [B, H, W]; K f64 [B, 3, 3]; Ra, Rb f64
 * [B, 3, 3]; ta, tb f64 [B, 3].  A row is NaN where either depth is non-finite or not positive.  src, dst f32 [B, N, 3]. */
int roma_op_depth_rows(const float* depth_a, const float* depth_b, const double* K, const double* Ra, const double* ta,
                       const double* Rb, const double* tb, int B, int H, int W, int step, float* out_src, float* out_dst,
                       void* stream);
/* Trajectory error: the camera centres -R^T t of R, t f64 [B, V, 3, 3], [B, V, 3] fitted to those of R_gt, t_gt by the closed
 * form (no truncation) over the views with view_ok u8 [B, V] (NULL: all).  Outputs: scale f64 [B], R f64 [B, 3, 3], t f64 [B, 3]
 * of the fit, centre_err f64 [B, V] (distance of the aligned centre to the true one), rot_err_deg f64 [B, V] (angle of
 * R_c R^T R_gt^T), rmse f64 [B] over the fitted views.  Fewer than 3 usable views or collinear centres: NaN everywhere. */
int roma_op_trajectory_error(const double* R, const double* t, const double* R_gt, const double* t_gt, const unsigned char* view_ok,
                             int B, int V, int with_scale, double* out_scale, double* out_r, double* out_t, double* out_centre_err,
                             double* out_rot_err_deg, double* out_rmse, void* stream);

#ifdef __cplusplus
}
#endif
#endif
