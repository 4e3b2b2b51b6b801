/* libroma_hip - the volumetric operators of the C ABI: a truncated signed distance volume (TSDF) that depth maps are integrated
 * into, and the triangle mesh of its zero level set.  What turns the fused depth maps of one or several reconstructions into one
 * surface, with no limit on the number of views: integration is additive, a second call goes on where the first stopped.
 * Defined in roma_amd/csrc/tsdf.hip, restated in numpy by tools/tsdf_ref.py.
 *
 * The declarations sit here, not in roma_hip.h (the table of ROMA_ABI_VERSION) and not in roma_hip_registration.h: both are
 * pinned entry by entry.  Both libraries export every name below; roma_amd/_lib.py binds them from this file (TSDF).
 *
 * Conventions as in roma_hip.h: DEVICE pointers unless stated otherwise; `stream` is a hipStream_t passed as void* (NULL = default
 * stream); calls are asynchronous on that stream; return 0 on success, negative on error (text: roma_last_error()).  Every
 * argument is checked before anything is enqueued.  R is row-major; x_cam = R X + t.
 *
 * A batch of B volumes shares (nz, ny, nx).  Voxel (k, j, i) of problem b - k along z, i along x, x fastest - has its centre at
 * origin[b] + (i + 0.5, j + 0.5, k + 0.5) * voxel_size[b]; origin f64 [B, 3], voxel_size f64 [B] and trunc f64 [B] (the truncation
 * distance in world units) are DEVICE data, so that a kernel can have made them.  A problem whose voxel_size or trunc is not
 * positive (or NaN) is left alone.  B nz ny nx, 7 nz ny nx and B V H W stay below 2^31.
 */
#ifndef ROMA_HIP_TSDF_H
#define ROMA_HIP_TSDF_H
#ifdef __cplusplus
extern "C" {
#endif

/* V views (1 <= V <= 8; more views are more calls) into the caller's volumes, in place.  tsdf f32 [B, nz, ny, nx] in units of
 * trunc, in [-1, 1]; weight f32 [B, nz, ny, nx]; color f32 [B, nz, ny, nx, 3] or NULL.  A fresh volume is tsdf 1, weight 0, color 0.
 * depth f32 [B, V, H, W] (NaN or <= 0: none; DenseFusion.depth as it is); depth_weight f32 [B, V, H, W] or NULL (1); cameras f64
 * [B, V, 3, 3] in grid units (the centre of cell (r, c) is (c + 0.5, r + 0.5)); R f64 [B, V, 3, 3], t f64 [B, V, 3]; view_valid u8
 * [B, V] or NULL; valid u8 [B] or NULL.  The colour source as roma_op_fuse_depth_maps takes it: images DEVICE u8, image_offsets HOST
 * long long [B, V], image_sizes HOST int [B, V, 2] = (h, w), all three or none, with color (then B V <= 128).
 * Every voxel takes the views in view order.  For a view: X the voxel centre in f64; (x, y, z) = R X + t, skipped unless z > near;
 * (u, v) = (fx x / z + cx, fy y / z + cy), the cell is (floor v, floor u), skipped outside the grid; d the cell's depth and w its
 * weight, skipped unless both are finite and positive; sdf = d - z in f64, skipped if sdf < -trunc; f = (float) min(1, sdf / trunc);
 * then in f32, operation by operation, tsdf = (weight * tsdf + w * f) / (weight + w), with colour and sdf <= trunc each channel of
 * color the same with the image pixel that holds the cell's centre in the place of f, and weight = min(weight + w, max_weight).
 * A pure function of its inputs in view order: bit-identical from run to run, independent of B, and the same whether the views
 * come in one call or in several. */
int roma_op_tsdf_integrate(const float* depth, const float* depth_weight, const double* cameras, const double* R, const double* t,
                           const unsigned char* view_valid, const unsigned char* valid, const unsigned char* images,
                           const long long* image_offsets, const int* image_sizes, const double* origin, const double* voxel_size,
                           const double* trunc, int B, int V, int H, int W, int nz, int ny, int nx, float max_weight, double near,
                           float* tsdf, float* weight, float* color, void* stream);
/* The zero level set by marching tetrahedra.  A voxel is valid when weight >= min_weight and inside when tsdf < 0.  Grid point
 * p = (i, j, k) owns the up to seven edges to p + d, d = (c & 1, c >> 1 & 1, c >> 2) for the edge class c = 1 .. 7; an edge carries one
 * vertex when both ends are valid and exactly one is inside: at s = f0 / (f0 - f1) along it (f64), stored as f32 world coordinates;
 * its colour c0 + s (c1 - c0) rounded to u8; its normal the normalised g0 + s (g1 - g0) of the central differences of tsdf at the
 * two ends, NaN when one of their six neighbours is outside the grid or not valid.  The cell at p (the cube to p + (1, 1, 1)) is
 * split into the six tetrahedra p, p + e_a, p + e_a + e_b, p + (1, 1, 1) over the permutations (a, b, c) of the axes in
 * lexicographic order; one whose four corners are valid emits 0, 1 or 2 triangles, wound so that (v1 - v0) x (v2 - v0) points to
 * the positive side.  Vertices are numbered in (grid point, edge class) order, faces in (cell, tetrahedron, triangle) order.
 * color f32 [B, nz, ny, nx, 3] or NULL, with out_colors.  Outputs: vertices, normals f32 [B, max_vertices, 3] (NaN padding), colors
 * u8 [B, max_vertices, 3] (0 padding), faces int32 [B, max_faces, 3] (-1 padding), counts int32 [B, 2] = min(totals, (max_vertices,
 * max_faces)), totals int32 [B, 2] = the vertices and faces there are, stats int32 [B, 8] = {valid voxels, inside ones, vertices
 * written, faces written, written vertices that no triangle uses (the rim of what was observed), faces written as (-1, -1, -1)
 * because they name a vertex beyond max_vertices, cells with a triangle, 0}.  Rows beyond the maxima are not written.  Nothing is
 * read back; bit-identical from run to run and independent of B.  workspace: device memory of
 * roma_op_tsdf_extract_mesh_workspace(B, nz, ny, nx, max_vertices) bytes; it need not be clear. */
long roma_op_tsdf_extract_mesh_workspace(int B, int nz, int ny, int nx, int max_vertices);
int roma_op_tsdf_extract_mesh(const float* tsdf, const float* weight, const float* color, const unsigned char* valid,
                              const double* origin, const double* voxel_size, int B, int nz, int ny, int nx, float min_weight,
                              int max_vertices, int max_faces, float* out_vertices, float* out_normals, unsigned char* out_colors,
                              int* out_faces, int* out_counts, int* out_totals, int* out_stats, void* workspace, long workspace_bytes,
                              void* stream);
/* The bounding box of the finite rows of points f32 [B, N, 3] below counts int32 [B] (NULL: N): out f64 [B, 2, 3] = (min, max), NaN
 * where a problem has no finite row.  One kernel; the minimum and maximum are taken over the ordered integer image of the float
 * bits, so the result does not depend on the order of arrival (-0 sorts below +0).  workspace: roma_op_points_bounds_workspace(B). */
long roma_op_points_bounds_workspace(int B);
int roma_op_points_bounds(const float* points, const int* counts, int B, int N, double* out, void* workspace, long workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
