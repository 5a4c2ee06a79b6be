"""mtgs_amd -- MI355X (gfx950) Gaussian-splatting rasterizer behind gsplat 1.4.0's Python API,
the hot path of OpenDriveLab/MTGS (rasterization() + spherical_harmonics()).

    from mtgs_amd import rasterization, spherical_harmonics      # or: `import gsplat` (shim package)

Importing this package does not load the HIP library or touch the GPU; the first operator call
does, and raises if libmtgs_rast.so has not been built (python -m mtgs_amd.build).

Beyond gsplat's surface: `mtgs_amd.graph_mode` / `mtgs_amd.graphs.GraphedIteration` (an iteration as one HIP graph launch),
`mtgs_amd.tight_lists` (opt-in shorter tile lists), `mtgs_amd.dist` (view-parallel data parallelism), `mtgs_amd.nodes` / `.loss`
/ `.densify` / `.optim` (the fused neighbours of the path), `mtgs_amd.appearance` (WildGaussians.py's appearance colours: `wild_colors`,
`wild_color_source`), `mtgs_amd.metrics` (get_metrics_dict's image metrics: `color_correct`, `image_metrics`), `mtgs_amd.seed`
(populate_modules: a node from a point cloud -- `knn_distances`, `seed_gaussians`, `sky_points`), `mtgs_amd.pointcloud`
(_load_3D_points: the cloud that node is seeded from -- `statistical_outlier_removal`, `voxel_down_sample`, `prepare_seed_cloud`),
`mtgs_amd.crop` (the viewer's and the render tool's crop box: `OrientedBox`, `crop_gaussians`), `mtgs_amd.densify.refine_scene`
(refinement_after for every node of the scene graph in one pass: `refine_scene`, `NodeRefine`, `RefineConfig`), `mtgs_amd.present`
(the last stage of the viewer and of the render tool -- colormaps, split / concatenated panels, uint8 frames, the viewer's resized
depth: `ColormapOptions`, `colorize`, `colorize_depth`, `viewer_frame`, `viewer_depth`, `render_frame`), `mtgs_amd.lpips` (the LPIPS
metric of get_metrics_dict, AlexNet on f32 MFMA: `LpipsWeights`, `mtgs_amd.metrics.lpips`, `image_metrics(..., lpips_weights=)`),
`mtgs_amd.dino` (the DINOv2 similarity metric, dinov2_sim: Pillow's resize and a ViT forward on the device -- `DinoConfig`, `DinoWeights`,
`dino_similarity`, `image_metrics(..., dino_weights=)`), `mtgs_amd.jpeg` (the presented frame as a baseline JPEG file, byte for byte
Pillow's: `encode_jpeg`, `JpegStream`, `viewer_frame(..., jpeg_quality=)`, `render_frame(..., jpeg_quality=)`), `mtgs_amd.jpegdec` (a baseline JPEG
file decoded on the device, byte for byte Pillow's pixels: `parse_jpeg`, `upload_jpeg`, `decode_jpeg`, `DeviceJpeg`, `JpegInfo`), `mtgs_amd.lidar` (lidar
sweeps through the cameras: the sparse lidar depth image of a frame and the colours and labels of the seeding cloud -- `depth_image`,
`paint_points`, `PaintedPoints`), `mtgs_amd.frame` (a training frame at its scale stage's resolution, byte for byte Pillow's BILINEAR and
NEAREST resize, and the masks of a frame: `resize_plane`, `resize_frame`, `frame_masks`, `masked_labels`, `scaled_size`), `mtgs_amd.stack` (the lidar sweeps of a traversal
split by the annotated boxes, painted and stacked into the background cloud and one cloud per tracked object: `split_sweep`,
`box_matrices`, `SweepStack`, `StackedClouds`), `mtgs_amd.registration` (the lidar sweeps of all traversals registered against a local
voxel map, KISS-ICP in a canonical order: `KissConfig`, `VoxelMap`, `LidarOdometry`, `register_traversals`, `align_points_to_map`,
`align_poses`, `registration_errors`), `mtgs_amd.undistort` (the lens undistortion of a training frame, one launch for every plane, by
a rule the project defines: `optimal_new_camera_matrix`, `undistort_camera`, `undistort_plane`, `undistort_frame`, `undistort_map`,
`UndistortCamera`), `mtgs_amd.brightness` (the cameras' brightness equalised: the V factors from the lidar overlap and the 8-bit HSV
adjust of V, one launch for a batch of images, by a rule the project defines: `adjust_brightness`, `estimate_brightness_factors`,
`pair_table`, `NUPLAN_PAIRS`; `SweepStack(equalise_brightness=True)`), `mtgs_amd.evaldump` (the evaluation image dump: a rendered frame
bent back into the raw camera and encoded, by a rule the project defines: `redistort_image`, `redistort_map`, `eval_dump`,
`eval_dump_paths`), `mtgs_amd.png` (depth and label planes as indexed PNG: a writer every PNG reader accepts and a parallel reader of
its files, with the reference's two depth rules fused in: `encode_png`, `encode_depth_png`, `PngStream`, `parse_png`, `upload_png`,
`decode_png`, `decode_depth_png`, `DevicePng`, `PngInfo`).
"""
from .appearance import wild_color_source, wild_colors
from .brightness import NUPLAN_PAIRS, adjust_brightness, estimate_brightness_factors, pair_table
from .crop import OrientedBox, crop_gaussians
from .densify import NodeRefine, RefineConfig, refine_scene
from .evaldump import eval_dump, eval_dump_paths
from .dino import DinoConfig, DinoWeights, dino_similarity
from .frame import frame_masks, masked_labels, resize_frame, resize_plane, scaled_size
from .jpeg import JpegStream, encode_jpeg
from .jpegdec import DeviceJpeg, JpegInfo, decode_jpeg, parse_jpeg, upload_jpeg
from .lidar import PaintedPoints, depth_image, paint_points
from .lpips import LpipsWeights
from .metrics import color_correct, image_metrics
from .present import ColormapOptions, colorize, colorize_depth, render_frame, viewer_depth, viewer_frame
from .png import DevicePng, PngInfo, PngStream, decode_depth_png, decode_png, encode_depth_png, encode_png, parse_png, upload_png
from .pointcloud import prepare_seed_cloud, statistical_outlier_removal, voxel_down_sample
from .registration import (KissConfig, LidarOdometry, VoxelMap, align_points_to_map, align_poses, register_traversals,
                           registration_errors)
from .rendering import rasterization
from .seed import knn_distances, seed_gaussians, sky_points
from .undistort import (UndistortCamera, optimal_new_camera_matrix, redistort_image, redistort_map, undistort_camera, undistort_frame,
                        undistort_map, undistort_plane)
from .stack import SplitSweep, StackedClouds, SweepStack, box_matrices, split_sweep
from .wrapper import (exact_lists, fully_fused_projection, graph_mode, isect_offset_encode, isect_tiles, lists_are_tight,
                      rasterize_to_pixels, sh_lazy, sh_prefill, spherical_harmonics, tight_lists)

__version__ = "0.1.0"
__all__ = ["rasterization", "spherical_harmonics", "fully_fused_projection", "isect_tiles",
           "isect_offset_encode", "rasterize_to_pixels", "graph_mode", "exact_lists", "tight_lists", "lists_are_tight", "sh_prefill", "sh_lazy",
           "wild_colors", "wild_color_source", "color_correct", "image_metrics", "knn_distances", "seed_gaussians", "sky_points",
           "statistical_outlier_removal", "voxel_down_sample", "prepare_seed_cloud", "OrientedBox", "crop_gaussians", "refine_scene", "NodeRefine", "RefineConfig",
           "ColormapOptions", "colorize", "colorize_depth", "viewer_frame", "viewer_depth", "render_frame", "LpipsWeights",
           "DinoConfig", "DinoWeights", "dino_similarity", "JpegStream", "encode_jpeg", "DeviceJpeg", "JpegInfo", "decode_jpeg", "parse_jpeg", "upload_jpeg", "depth_image", "paint_points", "PaintedPoints",
           "resize_plane", "resize_frame", "frame_masks", "masked_labels", "scaled_size",
           "split_sweep", "box_matrices", "SweepStack", "SplitSweep", "StackedClouds",
           "KissConfig", "VoxelMap", "LidarOdometry", "register_traversals", "align_points_to_map", "align_poses", "registration_errors",
           "UndistortCamera", "optimal_new_camera_matrix", "undistort_camera", "undistort_plane", "undistort_frame", "undistort_map",
           "adjust_brightness", "estimate_brightness_factors", "pair_table", "NUPLAN_PAIRS",
           "redistort_image", "redistort_map", "eval_dump", "eval_dump_paths",
           "encode_png", "encode_depth_png", "PngStream", "parse_png", "upload_png", "decode_png", "decode_depth_png", "DevicePng", "PngInfo"]
