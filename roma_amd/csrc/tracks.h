// Multi-view tracks from pairwise index matches (tracks.hip) and the N-view triangulation of tracks under given poses
// (triangulate_views.hip): the two stages between match_keypoints over the pairs of V <= 8 images and a V-view bundle_adjust.
// See roma_op_build_tracks / roma_op_triangulate_views in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
constexpr int ROMA_TRACKS_MAX_VIEWS = 8;        // views of one problem: ROMA_BA_MAX_VIEWS
constexpr int ROMA_TRACKS_MAX_KPTS = 1 << 16;   // keypoints per view: V K <= 2^19 nodes, four int32 a node in the workspace
constexpr int ROMA_TRACKS_MAX_PAIRS = 64;       // rows of pair_views: they travel in the kernel's arguments
constexpr int BUILD_TRACKS_INFO = 4;            // ints per problem in build_tracks_launch's out_info
constexpr int TRIANGULATE_VIEWS_STATS = 8;      // ints per problem in triangulate_views_launch's out_stats
constexpr int TRIANGULATE_VIEWS_MAX_GN = 10;    // Gauss-Newton steps per fit

size_t build_tracks_workspace_bytes(int B, int V, int K, int P, int M);
// pair_views is HOST memory, int32 [P, 2]: it is checked before any device work and passed by value.  Everything else as in
// include/roma_hip.h.
int build_tracks_launch(const int* inds, const int* pair_views, const int* match_counts, const int* num_kpts, const float* x, int B,
                        int V, int K, int P, int M, int T, int min_views, int* out_tracks, float* out_kpts, int* out_counts,
                        int* out_total, int* out_info, void* ws, size_t ws_bytes, hipStream_t s);

int triangulate_views_launch(const float* kpts, const double* K, const double* R, const double* t, const unsigned char* view_valid,
                             const int* counts, const unsigned char* valid, int B, int V, int N, double max_reproj,
                             double min_parallax, double max_depth, int min_views, int gn_steps, int trim, double* out_points,
                             float* out_reproj, unsigned char* out_used, float* out_parallax, unsigned char* out_flags,
                             int* out_stats, hipStream_t s);
}  // namespace roma
