"""rodynrf (robust-dynrf_amd): the MI355X-native ray-batch hot path of RoDynRF.

Hand-written HIP kernels for gfx950 behind a C ABI (include/rodynrf.h, librodynrf.so), exposed
through the reference's own call surface:

    TensorVMSplit, TensorVMSplit_TimeEmbedding     (models/tensoRF.py: forward, compute_densityfeature /
                                                    compute_appfeature / compute_blendingfeature / warp_coordinate,
                                                    get_forward_backward_scene_flow, density_L1, TV_loss_*, ...)
    sampleXYZ, raw2outputs, OctreeRender_trilinear_fast, induce_flow, render_3d_point   (renderer.py)
    generate_rays                                  (train.py ray-generation block)

Importing this package loads librodynrf.so and raises if it is missing: there is no fallback.
"""
from . import _lib
from .fields import TensorVMSplit, TensorVMSplit_TimeEmbedding, TensorBase, query_points
from .alpha import AlphaGridMask, apply_alpha_mask, scene_alpha_volume, scene_dense_alpha
from .mesh import (extract_isosurface, field_mesh, mesh_sequence, export_mesh, write_ply, read_ply, vertex_colors,
                   colored_mesh, point_cloud, contract_to_world, simplify_mesh, simplify_lattice, scene_mesh, scene_mesh_sequence,
                   scene_vertex_colors, colored_scene_mesh, atlas_layout, atlas_uv, bake_texels, bake_texture, textured_mesh,
                   write_obj, read_obj)
from .renderer import (sampleXYZ, raw2outputs, OctreeRender_trilinear_fast, sample_rays, render_rays, render_chunks,
                       induce_flow, induce_flow_single, render_3d_point, render_single_3d_point,
                       eff_distloss, flatten_eff_distloss, render_frame, psnr, RenderMaps, camera_rays, render_view,
                       render_path, path_time, ssim, MotionMaps, flow_to_image, delta_xyz_image, Tracks, track_points,
                       render_tracks, track_visibility, render_hits, hit_view, hits_from_planes, render_hit_tracks)
from .ray_utils import generate_rays, ids2pixel, pose_to_mtx
from .regularizers import TVLoss
from .losses import LossTerms
from ._lib import RdrfError
from .scene import Scene, evaluate, pack_poses
from .step import Trainer, scene_config, N_to_reso, cal_n_samples, resolution_stages

__all__ = ["atlas_layout", "atlas_uv", "bake_texels", "bake_texture", "textured_mesh", "write_obj", "read_obj", "scene_alpha_volume", "scene_dense_alpha", "scene_mesh", "scene_mesh_sequence", "scene_vertex_colors", "colored_scene_mesh", "simplify_mesh", "simplify_lattice", "render_hit_tracks", "render_hits", "hit_view", "hits_from_planes", "point_cloud", "contract_to_world", "query_points", "vertex_colors", "colored_mesh", "extract_isosurface", "field_mesh", "mesh_sequence", "export_mesh", "write_ply", "read_ply", "Tracks", "track_points", "render_tracks", "track_visibility", "AlphaGridMask", "apply_alpha_mask", "Scene", "evaluate", "pack_poses", "Trainer", "scene_config", "N_to_reso", "cal_n_samples", "resolution_stages", "MotionMaps", "flow_to_image", "delta_xyz_image", "render_frame", "psnr", "RenderMaps", "camera_rays", "render_view", "render_path", "path_time", "ssim", "TVLoss", "pose_to_mtx", "eff_distloss", "flatten_eff_distloss", "induce_flow", "induce_flow_single", "render_3d_point", "render_single_3d_point",
           "TensorVMSplit", "TensorVMSplit_TimeEmbedding", "TensorBase", "sampleXYZ", "raw2outputs",
           "OctreeRender_trilinear_fast", "sample_rays", "render_rays", "render_chunks", "generate_rays", "ids2pixel", "LossTerms",
           "RdrfError"]
