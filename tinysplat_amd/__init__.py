"""tinysplat_amd - MI355X-native (gfx950, HIP) drop-in for the render path of maxgillett/tinysplat.

Exports the names tinysplat imports from gsplat (tinysplat/splatting/rasterize.py:3-4,
model_gaussian.py:14) plus the render adapter.  ``tinysplat_amd.sh`` mirrors ``gsplat.sh``.
"""
from .ops import (deg_from_sh, num_sh_bases, opacity_compensation, project_gaussians, rasterize_gaussians,
                  spherical_harmonics)
from .extract import ExtractConfig, SurfacePoints, extract_surface_points, level_set_points
from .mesh import MeshConfig, TriangleMesh, extract_mesh, vertex_colors
from .simplify import SimplifyConfig, simplify_mesh
from .clean import CleanConfig, clean_mesh, mesh_components
from .dataset import Dataset
from .depth import DepthPriors, SparseDepth, match_scale, sparse_depth
from .jpeg import JpegEncoder, encode_jpeg
from .mcmc import (ExponentialLr, McmcConfig, McmcDensifier, inject_noise, mcmc_normals, mean_opacity, mean_scale,
                   relocation, sample_rows)
from .masks import TrainingMasks, combine_masks, dilate_ignored, mask_coverage, masks_from_labels
from .metrics import EvalResult, Evaluator, affine_color_fit, evaluate, holdout_split, image_metrics
from .appearance import AppearanceConfig, AppearanceModel
from .edit import (Sim3, box_mask, crop_gaussians, merge_models, orient_from_cameras, sh_rotation_matrices,
                   transform_camera, transform_cameras, transform_gaussians, transform_points)
from .fusion import FusionConfig, extract_mesh_tsdf, fuse_depth_maps, render_depth_alpha
from .init import PointCloud, from_pcd, knn_points, read_point_cloud_ply
from .pose import PoseConfig, PoseModel, pose_gradient, refine_pose, se3_exp, se3_log
from .rasterizer import GaussianRasterizer
from .scene import Scene
from .semantic import (LiftResult, SemanticMaps, gaussian_contributions, label_iou, labels_from_votes, lift_labels,
                       render_labels, select_gaussians)
from .surface import (DensitySamples, SurfaceConfig, SurfaceRegularizer, density_loss, density_parts, opacity_entropy,
                      sample_points)
from .synthetic import RGB2SH, SH2RGB
from .viewer import Viewer

__all__ = ["project_gaussians", "rasterize_gaussians", "spherical_harmonics", "num_sh_bases",
           "deg_from_sh", "GaussianRasterizer", "Scene", "RGB2SH", "SH2RGB", "PointCloud", "from_pcd", "knn_points",
           "read_point_cloud_ply", "SurfaceConfig", "SurfaceRegularizer", "opacity_entropy", "DensitySamples",
           "sample_points", "density_loss", "density_parts", "ExtractConfig", "SurfacePoints", "extract_surface_points",
           "level_set_points", "MeshConfig", "TriangleMesh", "extract_mesh", "vertex_colors", "SimplifyConfig",
           "simplify_mesh", "CleanConfig", "clean_mesh", "mesh_components", "Dataset", "Viewer", "encode_jpeg", "JpegEncoder",
           "image_metrics", "evaluate", "holdout_split", "Evaluator", "EvalResult", "DepthPriors", "SparseDepth", "match_scale",
           "sparse_depth", "FusionConfig", "fuse_depth_maps", "render_depth_alpha", "extract_mesh_tsdf", "SemanticMaps",
           "LiftResult", "lift_labels", "labels_from_votes", "gaussian_contributions", "select_gaussians", "render_labels",
           "label_iou", "McmcConfig", "McmcDensifier", "ExponentialLr", "sample_rows", "relocation", "inject_noise",
           "mcmc_normals", "mean_opacity", "mean_scale", "AppearanceConfig", "AppearanceModel", "affine_color_fit", "Sim3",
           "sh_rotation_matrices", "transform_gaussians", "transform_camera", "transform_cameras", "transform_points",
           "orient_from_cameras", "box_mask", "crop_gaussians", "merge_models", "PoseConfig", "PoseModel", "pose_gradient",
           "refine_pose", "se3_exp", "se3_log", "TrainingMasks", "masks_from_labels", "dilate_ignored", "combine_masks",
           "mask_coverage", "opacity_compensation"]
