// Limits shared by the multi-view stages between match_keypoints over the pairs of V <= 8 images and a V-view bundle_adjust:
// keypoints_from_matches (set_keypoints.hip), build_tracks (tracks.hip) and triangulate_views (triangulate_views.hip).
#pragma once

namespace roma {
constexpr int ROMA_TRACKS_MAX_VIEWS = 8;        // views of one problem: bundle.hip's ROMA_BA_MAX_VIEWS
constexpr int ROMA_TRACKS_MAX_KPTS = 1 << 16;   // keypoints per view: V K <= 2^19 nodes, four int32 a node in the workspace
constexpr int ROMA_TRACKS_MAX_PAIRS = 64;       // rows of pair_views: they travel in the kernel's arguments
}  // namespace roma
