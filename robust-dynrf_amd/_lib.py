"""ctypes binding of librodynrf.so (C ABI declared in include/rodynrf.h).

The library is the product: there is NO fallback.  If it is missing or fails to load the import
raises, and every op raises if the tensors are not on a HIP device.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# RDRF_DETERMINISTIC=1: the debugging twin (fixed-point gradient accumulation, bit-reproducible gradients; csrc/Makefile)
DETERMINISTIC = os.environ.get("RDRF_DETERMINISTIC", "0") == "1"
LIB_PATH = os.environ.get("RDRF_LIB", os.path.join(_HERE, "librodynrf_det.so" if DETERMINISTIC else "librodynrf.so"))  # RDRF_LIB: A/B builds

ABI_VERSION = 6   # include/rodynrf.h RDRF_ABI_VERSION: the parameter structs below are read to their full length

RAY_TYPES = {"ndc": 0, "contract": 1}   # any other name ("world") is RDRF_RAY_OTHER = 2: the world-space march
ACTS = {"relu": 0, "softplus": 1}
HEADS = {"MLP_Fea": 0, "MLP_Fea_TimeEmbedding": 1}
SAVE_NO_APP = 1   # include/rodynrf.h RDRF_SAVE_NO_APP (flags of rdrf_saved_bytes_ex / rdrf_*_fwd_ex)
QUERY_POINTS_MAX = 1 << 24   # include/rodynrf.h RDRF_QUERY_POINTS_MAX: the largest batch of one rdrf_query_points call
BAKE_TEXELS_MIN, BAKE_TEXELS_MAX = 4, 64   # include/rodynrf.h RDRF_BAKE_TEXELS_MIN / _MAX: the side of an atlas square

fp = C.POINTER(C.c_float)


class RdrfVM(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("line", C.c_void_p * 3), ("C", C.c_int * 3),
                ("H", C.c_int * 3), ("W", C.c_int * 3), ("L", C.c_int * 3),
                ("sH", C.c_int * 3), ("sW", C.c_int * 3)]


class RdrfFieldCfg(C.Structure):
    _fields_ = [("aabb", C.c_float * 6), ("distance_scale", C.c_float), ("weight_thres", C.c_float),
                ("density_shift", C.c_float), ("act", C.c_int), ("ray_type", C.c_int),
                ("static_head", C.c_int)]


class RdrfStaticParams(C.Structure):
    _fields_ = [("density", RdrfVM), ("app", RdrfVM), ("basis", C.c_void_p),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w3", C.c_void_p), ("b3", C.c_void_p), ("packed_fwd", C.c_void_p), ("packed_bwd", C.c_void_p)]


class RdrfDynamicParams(C.Structure):
    _fields_ = [("density", RdrfVM), ("blending", RdrfVM), ("app", RdrfVM), ("basis", C.c_void_p),
                ("rw1", C.c_void_p), ("rb1", C.c_void_p), ("rw2", C.c_void_p), ("rb2", C.c_void_p),
                ("rwv", C.c_void_p), ("rbv", C.c_void_p),
                ("l1w", C.c_void_p), ("l1b", C.c_void_p), ("l2w", C.c_void_p), ("l2b", C.c_void_p),
                ("l3w", C.c_void_p), ("l3b", C.c_void_p), ("l4w", C.c_void_p), ("l4b", C.c_void_p),
                ("l5w", C.c_void_p), ("l5b", C.c_void_p),
                ("dw1", C.c_void_p), ("db1", C.c_void_p), ("dw2", C.c_void_p), ("db2", C.c_void_p),
                ("bw1", C.c_void_p), ("bb1", C.c_void_p), ("bw2", C.c_void_p), ("bb2", C.c_void_p),
                ("sfw", C.c_void_p * 4), ("sfb", C.c_void_p * 4), ("packed_fwd", C.c_void_p), ("packed_bwd", C.c_void_p)]


class RdrfScatterTest(C.Structure):   # include/rodynrf.h RdrfScatterTest (rdrf_selftest_scatter)
    _fields_ = [("vm", RdrfVM * 2), ("gvm", RdrfVM * 2), ("set_mask", C.c_int), ("N", C.c_int), ("S", C.c_int), ("flat", C.c_int),
                ("coords", C.c_void_p), ("box_lo", C.c_float * 3), ("box_inv", C.c_float * 3), ("valid", C.c_void_p),
                ("list", C.c_void_p), ("count", C.c_void_p), ("rows", C.c_void_p), ("rows_floats", C.c_size_t),
                ("recs", C.c_void_p), ("recs_floats", C.c_size_t), ("dxw", C.c_void_p), ("g_xyz", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("keys_out", C.c_void_p), ("keys_sorted_out", C.c_void_p), ("order_out", C.c_void_p),
                ("counts_out", C.c_void_p)]


# RdrfRenderMaps (include/rodynrf.h): one nullable device pointer per per-ray output of the render, in this order
RENDER_MAPS = ("rgb", "depth", "acc", "rgb_s", "depth_s", "acc_s", "rgb_d", "depth_d", "acc_d", "blending")


class RenderMapsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RENDER_MAPS]


RENDER_MODES = {"auto": 0, "sequence": 1, "fused": 2}

# RdrfMotionMaps / RdrfMotionCams (include/rodynrf.h): the motion maps of the no-grad render and the cameras they project into
MOTION_MAPS = ("flow_f", "flow_b", "flow_s_f", "flow_s_b", "delta_xyz")


class MotionMapsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MOTION_MAPS]


class MotionCamsC(C.Structure):
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("focal", C.c_void_p), ("c2w_f", C.c_void_p), ("c2w_b", C.c_void_p),
                ("first_pixel", C.c_int64)]


# RdrfSceneTables / RdrfBatch (include/rodynrf.h): the tables of a device-resident training set and the tensors of one batch
class SceneTablesC(C.Structure):
    _fields_ = [("T", C.c_int), ("H", C.c_int), ("W", C.c_int), ("rgb_u8", C.c_int), ("rgb", C.c_void_p), ("disp", C.c_void_p),
                ("flow_f", C.c_void_p), ("flow_b", C.c_void_p), ("masks", C.c_void_p)]


BATCH_OUTPUTS = ("rgb", "disp", "fg", "mask_f", "mask_b", "flow_f", "flow_b", "ts", "ts_rand", "grid", "px", "view")


class BatchC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in BATCH_OUTPUTS]


# RdrfTrackCams / RdrfTracks (include/rodynrf.h): the cameras a point track is projected into and its nullable outputs
TRACK_OUTPUTS = ("pts", "pix", "disp")


class TrackCamsC(C.Structure):
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("K", C.c_int), ("focal", C.c_void_p), ("c2w", C.c_void_p)]


class TracksC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TRACK_OUTPUTS]


# RdrfHits (include/rodynrf.h): the nullable outputs of the surface hits, level-major
HIT_OUTPUTS = ("z", "hit", "xyz", "owner")
HITS_MAX_TAU = 8


class HitsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in HIT_OUTPUTS]


class RdrfAlphaMask(C.Structure):   # include/rodynrf.h RdrfAlphaMask: a packed occupancy grid (alpha.AlphaGridMask)
    _fields_ = [("bits", C.c_void_p), ("grid", C.c_int * 3), ("T", C.c_int), ("aabb", C.c_float * 6)]


# Every function include/rodynrf.h declares, in header order: name -> (restype, argtypes).  This is the one place a C
# signature is written down on the Python side; tests/test_abi_cpu.py holds it to the header's prototypes.  A pointer is
# c_void_p (it takes byref(struct), ptr(tensor), None, a raw data_ptr() and ctypes arrays alike) unless callers hand in a
# typed host pointer.
i32, u32, f32, usz, i64, vp = C.c_int, C.c_uint, C.c_float, C.c_size_t, C.c_int64, C.c_void_p
SIGNATURES = {
    "rdrf_abi_version": (i32, []),
    "rdrf_last_error": (C.c_char_p, []),
    "rdrf_workspace_bytes": (usz, [i32, i32]),
    "rdrf_forward_workspace_bytes": (usz, [i32, i32]),
    "rdrf_saved_bytes": (usz, [i32, i32, i32]),
    "rdrf_saved_bytes_ex": (usz, [i32, i32, i32, i32]),
    "rdrf_saved_row_bytes": (usz, [i32]),
    "rdrf_generate_rays": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp]),
    "rdrf_generate_rays_bwd": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]),
    "rdrf_generate_rays_uv": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp]),
    "rdrf_generate_rays_uv_bwd": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]),
    "rdrf_sample_ndc": (i32, [vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "rdrf_sample_contract": (i32, [vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "rdrf_sample_bwd": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    "rdrf_sample_world": (i32, [vp, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "rdrf_sample_world_bwd": (i32, [vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp]),
    "rdrf_static_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_static_fwd_ex": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, usz, vp, usz, vp, i32]),
    "rdrf_static_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, usz, vp, usz,
                             vp]),
    "rdrf_dynamic_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_dynamic_fwd_ex": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, usz, vp, usz, vp,
                                 i32]),
    "rdrf_dynamic_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, usz,
                              vp, usz, vp]),
    "rdrf_features_saved_bytes": (usz, [i32, i32]),
    "rdrf_features_workspace_bytes": (usz, [i32]),
    "rdrf_features_bwd_workspace_bytes": (usz, [i32]),
    "rdrf_static_features_fwd": (i32, [vp, vp, vp, i32, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_static_features_bwd": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_dynamic_features_fwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_dynamic_features_bwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_scene_flow_fwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_scene_flow_bwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, usz, vp, usz, vp]),
    "rdrf_composite_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "rdrf_composite_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "rdrf_induce_flow_fwd": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "rdrf_induce_flow_bwd": (i32, [i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "rdrf_rows_scatter_add": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "rdrf_distloss_fwd": (i32, [vp, vp, f32, vp, i32, i32, vp, vp]),
    "rdrf_distloss_bwd": (i32, [vp, vp, f32, vp, i32, i32, vp, vp, vp]),
    "rdrf_tv_fwd": (i32, [vp, i32, vp, vp]),
    "rdrf_tv_bwd": (i32, [vp, i32, vp, vp]),
    "rdrf_tv_grad": (i32, [vp, i32, vp, vp]),
    "rdrf_adam_step": (i32, [vp, vp, vp, vp, usz, usz, f32, f32, f32, f32, f32, i32, f32, vp]),
    "rdrf_upsample_bilinear": (i32, [vp, vp, i32, vp]),
    "rdrf_dense_l1_fwd": (i32, [vp, i32, f32, vp, vp]),
    "rdrf_dense_l1_bwd": (i32, [vp, vp, i32, f32, vp, vp]),
    "rdrf_pack_floats": (usz, []),
    "rdrf_static_pack": (i32, [vp, i32, i32, vp, vp]),
    "rdrf_dynamic_pack": (i32, [vp, i32, vp, vp]),
    "rdrf_loss_terms_workspace_floats": (usz, [i32]),
    "rdrf_loss_terms_fwd": (i32, [vp, i32, vp, vp, vp]),
    "rdrf_loss_terms_stats": (i32, [vp, i32, vp, vp, vp]),
    "rdrf_loss_terms_finish": (i32, [vp, i32, vp, vp, i32, vp, vp]),
    "rdrf_loss_terms_bwd": (i32, [vp, i32, vp, vp, vp]),
    "rdrf_frame_depth_loss_workspace_bytes": (usz, [i32, i32]),
    "rdrf_frame_depth_loss_fwd": (i32, [vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, usz, vp]),
    "rdrf_frame_depth_loss_bwd": (i32, [vp, vp, vp, i32, f32, vp, vp]),
    "rdrf_render_workspace_bytes": (usz, [i32, i32]),
    "rdrf_render_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, usz, vp]),
    "rdrf_render_fused_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, usz, vp]),
    "rdrf_render_sequence_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, usz, vp]),
    "rdrf_render_chunks_workspace_bytes": (usz, [i32, i32, i32]),
    "rdrf_render_chunks_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, usz, vp, vp, i32]),
    "rdrf_render_maps_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, i32, C.POINTER(RenderMapsC), vp, usz,
                                  vp]),
    "rdrf_render_chunks_maps_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, C.POINTER(RenderMapsC), vp,
                                         usz, vp, vp, i32]),
    "rdrf_render_world_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, i32, C.POINTER(RenderMapsC),
                                   vp, usz, vp, vp, i32]),
    "rdrf_render_motion_workspace_bytes": (usz, [i32, i32]),
    "rdrf_render_motion_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, i32, C.POINTER(RenderMapsC),
                                    C.POINTER(MotionCamsC), C.POINTER(MotionMapsC), vp, usz, vp]),
    "rdrf_flow_to_image_workspace_bytes": (usz, [i32, i32]),
    "rdrf_flow_to_image": (i32, [vp, i32, i32, vp, vp, usz, vp]),
    "rdrf_track_ws_bytes": (usz, [i32, i32]),
    "rdrf_track_points_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, C.POINTER(TrackCamsC), C.POINTER(TracksC), vp,
                                   usz, vp]),
    "rdrf_render_track_seeds_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, C.POINTER(RenderMapsC), vp, vp,
                                         usz, vp]),
    "rdrf_track_visibility_ws_bytes": (usz, [i32, i32, i32]),
    "rdrf_track_visibility_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, C.POINTER(TrackCamsC), i32, f32, f32,
                                       f32, vp, vp, usz, vp]),
    "rdrf_hits_from_planes": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, fp, i32, C.POINTER(HitsC), vp]),
    "rdrf_render_hits_ws_bytes": (usz, [i32, i32]),
    "rdrf_render_hits_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, fp, i32, C.POINTER(RenderMapsC),
                                  C.POINTER(HitsC), vp, usz, vp]),
    "rdrf_camera_rays": (i32, [vp, vp, i32, i32, i32, i32, f32, i64, i32, vp, vp]),
    "rdrf_ssim_workspace_bytes": (usz, [i32, i32, i32]),
    "rdrf_ssim": (i32, [vp, vp, i32, i32, i32, f32, vp, vp, vp, usz, vp]),
    "rdrf_gather_batch": (i32, [C.POINTER(SceneTablesC), vp, vp, i32, C.POINTER(BatchC), vp]),
    "rdrf_set_scatter_mode": (i32, [i32]),
    "rdrf_deterministic": (i32, []),
    "rdrf_det_bind": (i32, [i32, vp, usz, vp, vp]),
    "rdrf_det_finish": (i32, [i32, vp]),
    "rdrf_selftest_mlp": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, usz, vp]),
    "rdrf_selftest_layer": (i32, [i32, vp, vp, i32, i32, i32, vp, vp, usz, vp]),
    "rdrf_selftest_dw": (i32, [i32, i32, vp, usz, vp, usz, i32, vp, vp, vp]),
    "rdrf_selftest_dw_describe": (i32, [i32, i32, C.POINTER(C.c_int), i32]),
    "rdrf_selftest_dw_plan": (i32, [i32, i32, i32, C.POINTER(C.c_int), i32]),
    "rdrf_selftest_sf_geometry": (i32, [i32, vp, vp]),
    "rdrf_selftest_warp_geometry": (i32, [i32, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rdrf_selftest_warp_bwd_workspace_bytes": (usz, [i32, i32]),
    "rdrf_selftest_warp_bwd": (i32, [vp, vp, i32, i32, vp, usz, vp, usz, vp, vp, vp, vp, vp, vp, vp, vp, usz, vp]),
    "rdrf_selftest_sort_temp_bytes": (usz, [u32, i32]),
    "rdrf_selftest_sort": (i32, [vp, u32, i32, vp, u32, vp, vp, vp, usz, vp]),
    "rdrf_selftest_sort_seg_temp_bytes": (usz, [i32, u32, i32]),
    "rdrf_selftest_sort_seg": (i32, [vp, i32, u32, i32, vp, vp, vp, vp, usz, vp]),
    "rdrf_selftest_sort_describe": (i32, [i32, u32, i32, C.POINTER(C.c_ulong), i32]),
    "rdrf_selftest_scatter_workspace_bytes": (usz, [i32, i32]),
    "rdrf_selftest_scatter": (i32, [i32, i32, C.POINTER(RdrfScatterTest), vp]),
    "rdrf_selftest_scatter_describe": (i32, [i32, C.POINTER(C.c_int), C.POINTER(C.c_int), i32]),
    "rdrf_selftest_scatter_last": (i32, [C.POINTER(C.c_int), i32]),
    "rdrf_selftest_gather": (i32, [i32, vp, i32, vp, i32, vp, vp]),
    "rdrf_selftest_encodings": (i32, [vp, vp, i32, vp, vp, vp]),
    "rdrf_selftest_ray_scan": (i32, [i32, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
    "rdrf_selftest_ray_scan_bwd": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "rdrf_selftest_heads_bwd_workspace_bytes": (usz, [i32, i32]),
    "rdrf_selftest_heads_describe": (i32, [i32, i32, i32, C.POINTER(C.c_int), i32]),
    "rdrf_selftest_heads_bwd": (i32, [vp, vp, i32, i32, i32, vp, usz, vp, vp, vp, vp, i32, vp, usz, vp, usz, vp, vp, usz, vp]),
    "rdrf_selftest_time_branch": (i32, [vp, vp, i32, vp, vp, vp]),
    "rdrf_selftest_time_branch_bwd": (i32, [vp, vp, i32, i32, vp, vp, usz, vp, vp]),
    "rdrf_selftest_app_bwd_workspace_bytes": (usz, [i32, i32]),
    "rdrf_selftest_app_describe": (i32, [i32, i32, i32, i32, C.POINTER(C.c_int), i32]),
    "rdrf_selftest_app_bwd": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, usz, vp, vp, vp, vp, vp, vp, usz, vp, usz, vp, vp, vp, usz, vp]),
    "rdrf_compute_alpha_workspace_bytes": (usz, [i32, i32]),
    "rdrf_compute_alpha": (i32, [vp, i32, vp, vp, i32, vp, i32, f32, C.POINTER(RdrfAlphaMask), vp, vp, vp, usz, vp]),
    "rdrf_alpha_mask_build": (i32, [vp, i32, i32, i32, i32, f32, vp, vp, vp]),
    "rdrf_alpha_mask_sample": (i32, [C.POINTER(RdrfAlphaMask), vp, vp, i32, i64, vp, vp]),
    "rdrf_alpha_mask_valid": (i32, [C.POINTER(RdrfAlphaMask), C.POINTER(RdrfAlphaMask), vp, vp, i32, i32, vp, vp]),
    "rdrf_iso_ws_bytes": (usz, [i32, i32, i32]),
    "rdrf_iso_count": (i32, [vp, i32, i32, i32, i32, i32, f32, vp, usz, vp, vp]),
    "rdrf_iso_emit": (i32, [vp, i32, i32, i32, i32, i32, f32, vp, i32, vp, vp, vp, vp, i64, i64, vp]),
    "rdrf_render_masked_ws_bytes": (usz, [i32, i32]),
    "rdrf_render_masked_fwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, C.POINTER(RdrfAlphaMask),
                                    C.POINTER(RdrfAlphaMask), C.POINTER(RenderMapsC), vp, vp, usz, vp]),
    "rdrf_query_points_ws_bytes": (usz, [i32, i32, i32]),
    "rdrf_query_points": (i32, [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, usz, vp]),
    "rdrf_simplify_ws_bytes": (usz, [i64, i64, vp]),
    "rdrf_simplify_count": (i32, [vp, i64, vp, i64, vp, vp, vp, i32, vp, usz, vp, vp, vp]),
    "rdrf_simplify_emit": (i32, [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, i64, vp]),
    "rdrf_scene_alpha_ws_bytes": (usz, [i32, i32]),
    "rdrf_scene_alpha": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, f32, C.POINTER(RdrfAlphaMask), C.POINTER(RdrfAlphaMask), vp, vp,
                              vp, vp, vp, vp, usz, vp]),
    "rdrf_bake_texels": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "rdrf_bake_ws_bytes": (usz, [i32, i32, i32, i32]),
    "rdrf_bake_texture": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, usz, vp]),
    "rdrf_bake_scene_texture": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, f32, C.POINTER(RdrfAlphaMask),
                                     C.POINTER(RdrfAlphaMask), vp, i32, vp, vp, usz, vp]),
    "rdrf_prof_reset": (None, []),
    "rdrf_prof_enable": (i32, [i32]),
    "rdrf_prof_get": (i32, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
}
SYMBOLS = list(SIGNATURES)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C robust-dynrf_amd/csrc)")
    lib = C.CDLL(LIB_PATH)
    # the version check comes FIRST: a library of another version may lack symbols bound below, and the caller should see
    # "version mismatch", not a raw AttributeError
    version = getattr(lib, "rdrf_abi_version", None)
    got = version() if version is not None else None
    if got != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {got}, this binding is built against {ABI_VERSION} (include/rodynrf.h): rebuild "
                          "with make -C robust-dynrf_amd/csrc")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None)   # an A/B library of this version may predate an addition made inside it: skipped
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    if DETERMINISTIC and not lib.rdrf_deterministic():
        raise ImportError(f"RDRF_DETERMINISTIC=1 but {LIB_PATH} is the product build")
    return lib


lib = _load()


# rdrf_selftest_layer forms (include/rodynrf.h RDRF_ST_*)
SELFTEST_FORMS = {"F32": 0, "F32_T": 1, "B3": 2, "B3_T": 3, "B3_PAIR_T": 4, "B3S": 5, "B3S_T": 6}

# rdrf_selftest_dw plans and flags (include/rodynrf.h RDRF_DW_*)
DW_PLANS = {"DENSITY": 0, "STATIC_FEA": 1, "STATIC_TE": 2, "DYN_APP": 3, "DYN": 4, "SCENE_FLOW": 5, "FEAT_STATIC": 6, "FEAT_DYN": 7}
DW_LIVE_D, DW_LIVE_B, DW_SMALL_IN_KERNEL, DW_WARP_IN_KERNEL = 1, 2, 4, 8

# rdrf_selftest_scatter kinds (include/rodynrf.h RDRF_SCK_*)
SCATTER_KINDS = {"STATIC_DENSITY": 0, "DYN_DENSITY": 1, "STATIC_APP": 2, "DYN_APP": 3}

SCATTER_MODES = {"ray": 0, "sorted": 1, "auto": 2, "sorted_plain": 3}


def set_scatter_mode(mode):
    """rdrf_set_scatter_mode: "auto" (default: sorted from 300 k samples per launch) | "ray" | "sorted" | "sorted_plain"
    (sorted without the LDS plane windows of k_scatter_tiled) """
    check(lib.rdrf_set_scatter_mode(SCATTER_MODES[mode]), "rdrf_set_scatter_mode")


class RdrfTensor4(C.Structure):
    _fields_ = [("x", C.c_void_p), ("g", C.c_void_p), ("C", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("sC", C.c_longlong), ("sH", C.c_longlong), ("sW", C.c_longlong)]


TV_MAX = 16


class RdrfLossTerm(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("w", C.c_void_p), ("gx", C.c_void_p), ("gy", C.c_void_p),
                ("rows", C.c_longlong), ("cols", C.c_int), ("kind", C.c_int), ("norm", C.c_int),
                ("ysign", C.c_float), ("coef", C.c_float), ("coef_dev", C.c_void_p)]


MAX_LOSS_TERMS = 32


class RdrfError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise RdrfError(f"{what} failed (rc={rc}): {lib.rdrf_last_error().decode()}")


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RdrfError("rodynrf ops run on the MI355X only: got a CPU tensor "
                            "(there is no CPU fallback; the oracle lives under oracle/ for tests)")


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream_of(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


_ws = {}          # (device, stream) -> scratch buffer, most recently used last
_WS_MAX = 20      # the default stream + the 16 side streams of render_chunks + slack: older entries are dropped


def workspace(device, nbytes):
    """scratch of the C entry points, one buffer per (device, stream): calls on different streams (render_chunks) must
    not share scratch.  The cache is an LRU of _WS_MAX entries (a stream that is no longer used gives its buffer back to
    the caching allocator, which keeps it ordered behind that stream's work); growing a buffer drops the old one first."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws.pop(key, None)
    if buf is None or buf.numel() < nbytes:
        buf = None   # free before allocating: the peak is one buffer, not two
        buf = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
    _ws[key] = buf
    while len(_ws) > _WS_MAX:
        _ws.pop(next(iter(_ws)))
    return buf


def release_workspaces():
    """drop every cached scratch buffer (they return to torch's caching allocator)"""
    _ws.clear()


def zeros_like_many(tensors, want=None):
    """torch.zeros_like for several tensors with ONE fill launch: contiguous fp32 views (256-byte aligned) of a
    single zeroed buffer; entries that are None (or whose `want` flag is false) come back as None."""
    want = [t is not None for t in tensors] if want is None else [bool(w) and t is not None for t, w in zip(tensors, want)]
    sizes = [((t.numel() + 63) // 64) * 64 if w else 0 for t, w in zip(tensors, want)]
    total = sum(sizes)
    if total == 0:
        return [None] * len(tensors)
    dev = next(t.device for t, w in zip(tensors, want) if w)
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    out, o = [], 0
    for t, w, n in zip(tensors, want, sizes):
        out.append(flat[o: o + t.numel()].view(t.shape) if w else None)
        o += n
    return out


def f32c(t):
    """contiguous fp32 view (no copy when already so)"""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
