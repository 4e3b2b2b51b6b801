// The pair_views argument of fuse_depth_maps, relative_poses, keypoints_from_matches and build_tracks: P rows (view a, view b),
// checked on the host and handed to the kernels as a byte table inside their arguments.
#pragma once
#include "common.h"

namespace roma {

// both views of every pair in range and different; fills pv.  `op` prefixes the messages.
inline int check_pairs(const char* op, const int* pair_views, int V, int P, unsigned char (*pv)[2]) {
  for (int p = 0; p < P; ++p) {
    const int a = pair_views[2 * p], c = pair_views[2 * p + 1];
    ROMA_REQUIRE(a >= 0 && a < V && c >= 0 && c < V, std::string(op) + ": pair_views entry out of range [0, V)");
    ROMA_REQUIRE(a != c, std::string(op) + ": pair_views joins a view to itself");
    pv[p][0] = (unsigned char)a, pv[p][1] = (unsigned char)c;
  }
  return 0;
}

}  // namespace roma
