"""roma_amd - MI355X-native RoMa dense matching (`RegressionMatcher.match()` hot path).

Public surface mirrors the reference package (`romatch/__init__.py:2`): model factories and the
local-correlation operator, plus the post-processing of `sample()` output (robust homography /
fundamental / essential-matrix estimation, relative and absolute pose, bundle adjustment).  Everything numerical runs in libroma_hip.so (hand-written HIP, gfx950).
"""
from .matcher import RegressionMatcher, roma_indoor, roma_model, roma_outdoor  # noqa: F401
from .local_correlation import local_corr, local_correlation  # noqa: F401
from .kde import kde  # noqa: F401
from .sampling import multinomial, sample_matches  # noqa: F401
from .geometry import (essential_magsac, essential_minimal, estimate_pose, estimate_pose_uncalibrated, find_essential,  # noqa: F401
                       find_fundamental, find_homography, magsac, recover_pose, refine_fundamental, refine_homography, refine_pose)
from .absolute_pose import absolute_pose_minimal, estimate_absolute_pose, lift_matches, refine_absolute_pose  # noqa: F401
from .registration import (Similarity, TrajectoryError, align_points, apply_similarity, depth_rows, fit_similarity,  # noqa: F401
                           refine_similarity, register_depth_maps, similarity_minimal, trajectory_error)
from .bundle import BundleResult, ViewsReconstruction, bundle_adjust, reconstruct_pair, reconstruct_views  # noqa: F401
from .triangulation import ViewsTriangulation, depth_consistency, triangulate, triangulate_views, triangulate_warp  # noqa: F401
from .tracks import Tracks, build_tracks  # noqa: F401
from .set_keypoints import SetKeypoints, keypoints_from_matches  # noqa: F401
from .depth_fusion import DenseFusion, fuse_depth_maps, relative_poses  # noqa: F401
from .point_render import PointRender, orbit_cameras, render_points  # noqa: F401
from .tsdf import (Mesh, TSDFVolume, extract_mesh, integrate_depth_maps, mesh_from_fusion, points_bounds, tsdf_bounds,  # noqa: F401
                   tsdf_volume, write_ply)
from .preprocess import preprocess_images  # noqa: F401
from .encoded import EncodedImages, all_pairs, pack_layout  # noqa: F401
from .gt_warp import DenseMetrics, dense_metrics, get_gt_warp, warp_kpts  # noqa: F401
from .metrics import (ErrorLog, ErrorSummary, PoseError, compute_pose_error, homography_corner_error,  # noqa: F401
                      hpatches_coordinates, pose_auc, pose_error)
from .render import morph_times, render_morph  # noqa: F401
from .keypoints import KeypointMatches, match_keypoints  # noqa: F401
from .tiny import TinyRoMa, tiny_roma_v1_outdoor  # noqa: F401

__all__ = ["pose_error", "compute_pose_error", "homography_corner_error", "pose_auc", "ErrorLog", "ErrorSummary", "PoseError",
           "hpatches_coordinates", "match_keypoints", "KeypointMatches", "render_morph", "morph_times", "warp_kpts", "get_gt_warp", "dense_metrics", "DenseMetrics", "preprocess_images", "triangulate", "triangulate_warp", "depth_consistency",
"RegressionMatcher", "roma_model", "roma_outdoor", "roma_indoor", "local_corr", "local_correlation", "kde",
           "multinomial", "sample_matches", "find_homography", "find_fundamental", "find_essential", "recover_pose", "refine_pose", "estimate_pose",
           "refine_homography", "refine_fundamental", "estimate_pose_uncalibrated", "essential_minimal", "magsac", "essential_magsac",
           "estimate_absolute_pose", "absolute_pose_minimal", "refine_absolute_pose", "lift_matches",
           "Similarity", "TrajectoryError", "align_points", "similarity_minimal", "refine_similarity", "fit_similarity",
           "apply_similarity", "depth_rows", "register_depth_maps", "trajectory_error",
           "bundle_adjust", "reconstruct_pair", "BundleResult", "build_tracks", "Tracks", "triangulate_views", "ViewsTriangulation",
           "reconstruct_views", "ViewsReconstruction", "keypoints_from_matches", "SetKeypoints",
           "fuse_depth_maps", "relative_poses", "DenseFusion",
           "render_points", "orbit_cameras", "PointRender",
           "tsdf_volume", "tsdf_bounds", "points_bounds", "integrate_depth_maps", "extract_mesh", "mesh_from_fusion", "write_ply",
           "TSDFVolume", "Mesh",
           "EncodedImages", "all_pairs", "pack_layout",
           "TinyRoMa", "tiny_roma_v1_outdoor"]
