// The `model` codes of roma_op_ransac / roma_op_magsac (geometry.hip) and roma_op_refine_model (model_refine.hip).
#pragma once

namespace roma {
constexpr int RANSAC_HOMOGRAPHY = 0, RANSAC_FUNDAMENTAL = 1;
}  // namespace roma
