// Triangulation of matches under a known relative pose, and the depth consistency of the two halves of a symmetric warp:
// see triangulate.hip and roma_op_triangulate / roma_op_depth_consistency in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
// flag bits of roma_op_triangulate (tools/triangulate_ref.py: the same names)
constexpr unsigned char TRI_SKIPPED = 1, TRI_DEGENERATE = 2, TRI_CHEIRALITY = 4, TRI_REPROJ = 8, TRI_PARALLAX = 16, TRI_CERTAINTY = 32;

int triangulate_launch(const float* matches, const float* certainty, const int* counts, const unsigned char* valid, const double* R,
                       const double* t, const double* K_a, const double* K_b, int B, long n, int coords, int W_a, int H_a, int W_b,
                       int H_b, int sym_w, double max_depth, double max_reproj, double min_parallax, double min_certainty,
                       float* points, float* depth_other, float* reproj, float* parallax, unsigned char* flags, int* stats,
                       hipStream_t s);
int depth_consistency_launch(const float* points, const unsigned char* flags, const double* R, const double* t, const double* K_a,
                             const double* K_b, int W_a, int H_a, int W_b, int H_b, int B, int H, int W, double rel_thresh,
                             unsigned char* consistent, float* err, hipStream_t s);
}  // namespace roma
