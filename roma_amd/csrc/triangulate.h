// The flag bits of roma_op_triangulate (triangulate.hip), which roma_op_triangulate_views (triangulate_views.hip) shares.
#pragma once

namespace roma {
// tools/triangulate_ref.py: the same names
constexpr unsigned char TRI_SKIPPED = 1, TRI_DEGENERATE = 2, TRI_CHEIRALITY = 4, TRI_REPROJ = 8, TRI_PARALLAX = 16, TRI_CERTAINTY = 32;
}  // namespace roma
