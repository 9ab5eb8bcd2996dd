"""ctypes binding of libtinysplat_hip.so (the C ABI declared in include/tinysplat_hip.h).

There is no fallback: if the shared library is missing or does not export the full ABI, importing
the ops raises.  Build it with ``python -m tinysplat_amd._build`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_double, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p
from pathlib import Path

# TS_LIB_PATH: another build of the library (tests/test_gpu_variants.py loads builds with the other settings of the
# compile-time switches in a process of their own); a variant build needs TS_ALLOW_VARIANT_LIB=1 as usual
LIB_PATH = Path(os.environ["TS_LIB_PATH"]) if os.environ.get("TS_LIB_PATH") else \
    Path(__file__).resolve().parent / "csrc" / "libtinysplat_hip.so"
ABI_VERSION = 9
HINT_BALANCED_WALK = 1           # ts_camera.hints: TS_HINT_BALANCED_WALK
HINT_COOP_SPLIT = 1 << 20        # ts_camera.hints: TS_HINT_COOP_SPLIT
# the header's TS_RASTER_* and TS_FRAME_* flag bits under the same names (tests/test_abi.py compares them)
RASTER_LOGIT_OPACITY = 1
RASTER_CLAMP_RGB = 2
RASTER_SPLIT_BLOCKS = 4
RASTER_NARROW_WAVES = 8
FRAME_TIGHT = 1
FRAME_SPLIT = 2
FRAME_NARROW_WAVES = 8
FRAME_STRIPE = 16
FRAME_DIRECT_SCATTER = 32
FRAME_PLANES = 64
FRAME_SEPARATE_SORT = 128
FRAME_LIST_STATS = 256
FRAME_SURVIVORS = 512
FRAME_GROUP_COUNTS = 1024
FRAME_ONE_WALK = 2048
FRAME_ROW_SPANS = 4096
FRAME_LINEAR_OPACITY = 8192
PARTIAL_ROW_FLOATS = 12          # TS_PARTIAL_ROW_FLOATS: floats per (tile, Gaussian) gradient row slot


class TsCamera(ctypes.Structure):
    """struct ts_camera of include/tinysplat_hip.h."""
    _fields_ = [
        ("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float),
        ("img_width", c_int32), ("img_height", c_int32),
        ("tile_bounds_x", c_int32), ("tile_bounds_y", c_int32),
        ("tile_row0", c_int32), ("tile_rows", c_int32),
        ("glob_scale", c_float), ("clip_thresh", c_float),
        ("wide_tiles", c_int32), ("hints", c_int32),
    ]


_P = c_void_p  # every device pointer travels as an integer address
_CAM = POINTER(TsCamera)


class TsDensifyPolicy(ctypes.Structure):
    """ts_densify_policy of include/tinysplat_hip.h."""
    _fields_ = [("interval_densify", c_float), ("max_dim", c_float), ("tau_means", c_float),
                ("scale_thresh", c_float)]


class TsFrame(ctypes.Structure):
    """struct ts_frame of include/tinysplat_hip.h: one frame of the adapter recipe for the native
    executor (ts_frame_*).  Pointers travel as integer addresses; unset ones stay NULL."""
    _fields_ = ([("n", c_int32), ("num_bases", c_int32), ("sh_degree", c_int32), ("channels", c_int32),
                 ("flags", c_int32), ("flag_gen", c_int32), ("cam", TsCamera)]
                + [(name, c_void_p) for name in (
                    "means", "scales", "quats", "opacities", "colors_dc", "colors_rest",
                    "view34", "projview", "origin", "background",
                    "xys", "depths", "conics", "colors", "splats",
                    "radii", "num_tiles_hit", "cum_tiles_hit", "sh_mask",
                    "scan_ws", "bin_ws", "tile_bins", "total_host")]
                + [("num_intersects", c_int64), ("capacity", c_int64)]
                + [(name, c_void_p) for name in (
                    "bucket_ids", "gaussian_ids_sorted", "out_img", "final_Ts", "final_index", "clamp_mask",
                    "v_out_img", "partials", "row_flags",
                    "v_xy", "v_conic", "v_colors", "v_depth", "v_opacity",
                    "v_means", "v_scales", "v_quats", "v_colors_dc", "v_colors_rest",
                    "out_depth", "v_out_depth", "survivors", "row_spans")])


_FRAME = POINTER(TsFrame)


class TsAdam(ctypes.Structure):
    """struct ts_adam: the optimiser state the fused parameter-stage backward updates (groups in the order of
    SplatModel.parameters(): means, colors_dc, colors_rest, scales, quats, opacities)."""
    _fields_ = [("exp_avg", c_void_p * 6), ("exp_avg_sq", c_void_p * 6), ("lr", c_float * 6), ("step", c_int32 * 6),
                ("beta1", c_float), ("beta2", c_float), ("eps", c_float)]


_ADAM = POINTER(TsAdam)

MAX_RANKS = 16


class TsStripes(ctypes.Structure):
    """struct ts_stripes: rank d renders tile rows [row[d], row[d+1])."""
    _fields_ = [("num", c_int32), ("row", c_int32 * (MAX_RANKS + 1))]


_STRIPES = POINTER(TsStripes)


class TsRankStep(ctypes.Structure):
    """struct ts_rank_step: what the four ts_shard_rank_* calls of one rank's step share."""
    _fields_ = [("stripes", TsStripes), ("group_base", c_int32 * (MAX_RANKS + 1)), ("gid_base", c_int32),
                ("send_rows", c_int32), ("recv_rows", c_int32), ("route_ws", c_void_p), ("counts", c_void_p),
                ("send", c_void_p), ("recv", c_void_p), ("grad_rows", c_void_p), ("back", c_void_p)]


_RANK = POINTER(TsRankStep)

TSDF_NO_CULL = 1                 # TS_TSDF_NO_CULL
TSDF_PLANES = 6                  # TS_TSDF_PLANES, of TS_TSDF_PLANE_FLOATS = 5 floats each


class TsTsdfCamera(ctypes.Structure):
    """struct ts_tsdf_camera of csrc/tsdf_math.h: one record of the fusion's device table."""
    _fields_ = [("view", c_float * 12), ("proj", c_float * 12), ("planes", c_float * (TSDF_PLANES * 5)),
                ("width", c_int32), ("height", c_int32), ("depth", c_void_p)]


LOSS_MASKED = 1                  # TS_LOSS_MASKED


class TsLoss(ctypes.Structure):
    """struct ts_loss of include/tinysplat_hip.h: the training loss on any image layout, with or without a mask.
    Pointers travel as integer addresses; unset ones stay NULL."""
    _fields_ = ([("height", c_int32), ("width", c_int32), ("pixel_floats", c_int32), ("flags", c_int32)]
                + [(name, c_void_p) for name in ("image", "depth", "target", "depth_target", "mask")]
                + [("w_l1", c_float), ("w_ssim", c_float), ("w_depth", c_float)]
                + [(name, c_void_p) for name in ("ws", "v_image", "v_depth")])


ENTRY_PROBE = ctypes.CFUNCTYPE(None, ctypes.c_char_p, c_int32, c_void_p)      # ts_entry_probe

# name -> (restype, argtypes); mirrors include/tinysplat_hip.h declaration by declaration
SIGNATURES = {
    "ts_abi_version": (c_int32, []),
    "ts_project_fwd": (c_int32, [c_int32, _P, _P, _P, _P, _P, _CAM, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_project_bwd": (c_int32, [c_int32, _P, _P, _P, _P, _P, _CAM, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_sh_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "ts_sh_bwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "ts_sh_colors_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_sh_colors_bwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_scan_ws_ints": (c_int64, [c_int32]),
    "ts_scan_tiles": (c_int32, [c_int32, _P, _P, _P, _P, _P]),
    "ts_bin_ws_ints": (c_int64, [c_int32, c_int32]),
    "ts_bin_count": (c_int32, [c_int32, _P, _P, _P, _CAM, _P, _P]),
    "ts_tile_offsets": (c_int32, [c_int32, c_int32, _P, _P, _P, c_int64, _P]),
    "ts_tile_offsets_stats": (c_int32, [c_int32, c_int32, _P, _P, _P, c_int64, _P, _P]),
    "ts_bin_scatter": (c_int32, [c_int32, _P, _P, _P, _CAM, _P, _P, _P, _P]),
    "ts_sort_tiles": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_sort_tiles_above": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_bin_group_form": (c_int32, [c_int32]),
    "ts_bin_count_groups": (c_int32, [c_int32, _P, _P, _P, _CAM, _P, _P]),
    "ts_group_offsets": (c_int32, [c_int32, c_int32, _P, _P, _P, c_int64, _P, _P]),
    "ts_bin_scatter_groups": (c_int32, [c_int32, _P, _P, _P, _CAM, _P, _P, _P, _P, _P]),
    "ts_bin_one_walk_form": (c_int32, [c_int32, c_int32]),
    "ts_bin_stage_capacity": (c_int32, []),
    "ts_bin_emit_groups": (c_int32, [c_int32, _P, _P, _P, _CAM, _P, c_int64, _P, _P, _P]),
    "ts_bin_emit_groups_spans": (c_int32, [c_int32, _P, _P, _P, _P, _CAM, _P, c_int64, _P, _P, _P]),
    "ts_emit_offsets": (c_int32, [c_int32, c_int32, _P, _P, _P, c_int64, _P, _P]),
    "ts_bin_gather_groups": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P]),
    "ts_sort_tiles_stats": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, c_int32, _P, _P, _P]),
    "ts_sort_tiles_above_stats": (c_int32, [c_int32, _P, _P, _P, _P, c_int32, _P, _P, _P]),
    "ts_num_tiles": (c_int32, [_CAM]),
    "ts_final_floats": (c_int64, [_CAM, c_int32]),
    "ts_cut_tiles": (c_int32, [_CAM, _P, _P]),
    "ts_colors_pack_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, c_int32, c_int32,
                                     _P, _P, _P, _P, _P, _CAM, _P, _P, _P]),
    "ts_colors_pack_spans_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, c_int32, c_int32,
                                           _P, _P, _P, _P, _P, _CAM, _P, _P, c_int32, _P, _P]),
    "ts_pack_splats": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _CAM, _P, _P, _P]),
    "ts_raster_fwd": (c_int32, [c_int32, c_int32, _CAM, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_raster_bwd": (c_int32, [c_int32, c_int32, c_int64, _CAM, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_raster_fwd_planes": (c_int32, [c_int32, c_int32, _CAM, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_raster_fwd_sort": (c_int32, [c_int32, c_int32, _CAM, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_raster_bwd_planes": (c_int32, [c_int32, c_int32, c_int64, _CAM, _P, _P, _P, _P, _P, _P, _P, _P, c_int32,
                                       _P, _P, _P, _P, _P]),
    "ts_bench_stream_read": (c_int32, [_P, c_int64, _P, _P]),
    "ts_bench_gather48": (c_int32, [_P, _P, c_int64, _P, _P]),
    "ts_photometric_ws_floats": (c_int64, [c_int32, c_int32]),
    "ts_loss_struct_bytes": (c_int32, []),
    "ts_photometric_loss_rgbd": (c_int32, [POINTER(TsLoss), _P]),
    "ts_photometric_loss_reduce": (c_int32, [c_int32, c_int32, c_float, c_float, c_float, _P, _P, _P]),
    "ts_mask_blend": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P]),
    "ts_adam_step": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, _P, c_float, c_float, c_float, _P]),
    "ts_sh_colors_bwd_adam": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _ADAM, _P]),
    "ts_project_bwd_adam": (c_int32, [c_int32, _P, _P, _P, _P, _P, _CAM, c_int32, _P, _P, _P, _P, _P, _P, _ADAM, _P]),
    "ts_frame_bwd_params_adam": (c_int32, [_FRAME, _ADAM, _P]),
    "ts_grad_accum": (c_int32, [c_int32, _P, _P, _P]),
    "ts_densify_classify": (c_int32, [c_int32, _P, _P, _P, POINTER(TsDensifyPolicy), _P, _P]),
    "ts_densify_ws_ints": (c_int64, [c_int32]),
    "ts_densify_plan": (c_int32, [c_int32, _P, _P, _P, _P, _P]),
    "ts_gather_rows": (c_int32, [c_int32, _P, _P, _P, c_int32, c_int32, _P, _P]),
    "ts_split_fixup": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_ply_row_floats": (c_int32, [c_int32]),
    "ts_ply_pack_rows": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_ply_unpack_rows": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_reduce_partials": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_route_ws_ints": (c_int64, [c_int32, c_int32]),
    "ts_route_count": (c_int32, [c_int32, _P, _P, _CAM, _STRIPES, _P, _P, _P]),
    "ts_route_count_padded": (c_int32, [c_int32, _P, _P, _CAM, _STRIPES, _P, _P, _P, _P]),
    "ts_route_pack": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _CAM, _STRIPES, _P, _P, _P]),
    "ts_import_records": (c_int32, [c_int32, _P, _CAM, _P, _P, _P, _P, _P]),
    "ts_import_pack": (c_int32, [c_int32, _P, _P, _CAM, _P, _P]),
    "ts_reduce_partials_rows": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_route_accumulate": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _CAM, _STRIPES, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_shard_owner_fwd": (c_int32, [_FRAME, _STRIPES, _P, _P, _P]),
    "ts_shard_owner_fwd_padded": (c_int32, [_FRAME, _STRIPES, _P, _P, _P, _P]),
    "ts_shard_owner_fwd_fused": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _CAM, c_int32, _P, _P, _P, _P,
                                           c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _STRIPES, _P, _P, _P, _P]),
    "ts_shard_owner_bwd_fused": (c_int32, [c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                           _CAM, _STRIPES, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_shard_stripe_fwd_import": (c_int32, [_FRAME, _P, _P]),
    "ts_shard_stripe_bwd": (c_int32, [_FRAME, _P, _P]),
    "ts_shard_owner_bwd": (c_int32, [_FRAME, _STRIPES, _P, _P, _P]),
    "ts_rank_step_struct_bytes": (c_int32, []),
    "ts_shard_rank_fwd_a": (c_int32, [_FRAME, _RANK, _P]),
    "ts_shard_rank_fwd_b": (c_int32, [_FRAME, _RANK, _P]),
    "ts_shard_rank_bwd_a": (c_int32, [_FRAME, _RANK, _P]),
    "ts_shard_rank_bwd_b": (c_int32, [_FRAME, _RANK, _P]),
    "ts_frame_struct_bytes": (c_int32, []),
    "ts_frame_fwd_project": (c_int32, [_FRAME, _P]),
    "ts_frame_fwd_prepare": (c_int32, [_FRAME, _P]),
    "ts_frame_fwd_composite": (c_int32, [_FRAME, _P]),
    "ts_frame_bwd_composite": (c_int32, [_FRAME, _P]),
    "ts_frame_bwd_params": (c_int32, [_FRAME, _P]),
    "ts_set_entry_probe": (c_int32, [_P, _P]),       # (an ENTRY_PROBE instance, or None)
    "ts_knn_ws_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "ts_knn": (c_int32, [c_int32, _P, c_int32, _P, c_int32, _P, _P, _P, _P, _P]),
    "ts_init_from_points": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_opacity_entropy_ws_bytes": (c_int64, [c_int32]),
    "ts_opacity_entropy": (c_int32, [c_int32, _P, _P, _P, _P, _P]),
    "ts_density_sample_ws_bytes": (c_int64, [c_int32]),
    "ts_density_sample": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_density_loss_ws_bytes": (c_int64, [c_int32]),
    "ts_density_loss": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, _P, _P, c_int32,
                                  c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_segment_sum_ws_bytes": (c_int64, [c_int64, c_int32]),
    "ts_segment_sum": (c_int32, [c_int64, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_extract_pack": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_extract_rays": (c_int32, [c_int32, _P, c_int32, c_int32, _P, c_int32, _P, _P, _P, _P, _P, _P]),
    "ts_extract_samples": (c_int32, [c_int32, c_int32, c_int32, c_float, _P, _P, _P, _P, _P, _P, _P]),
    "ts_extract_march": (c_int32, [c_int32, c_int32, c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                   _P, _P, _P]),
    "ts_extract_normals": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P]),
    "ts_extract_chunk_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "ts_mesh_boxes": (c_int32, [c_int32, _P, _P, _P, c_float, _P, _P]),
    "ts_mesh_mark": (c_int32, [c_int32, _P, _P, _P, _P, _P]),
    "ts_mesh_chunk_bytes": (c_int64, [c_int32, c_int32]),
    "ts_mesh_corners": (c_int32, [c_int32, _P, _P, _P, _P, _P]),
    "ts_mesh_density": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_mesh_count": (c_int32, [c_int32, _P, _P, _P, c_float, _P, _P, _P]),
    "ts_mesh_emit": (c_int32, [c_int32, _P, _P, _P, c_float, _P, _P, _P, _P, _P, _P]),
    "ts_tsdf_camera_bytes": (c_int32, []),
    "ts_tsdf_mark": (c_int32, [c_int32, _P, c_int64, _P, _P, c_float, c_float, _P, _P]),
    "ts_tsdf_chunk_bytes": (c_int64, [c_int32]),
    "ts_tsdf_integrate": (c_int32, [c_int32, _P, _P, _P, _P, c_int32, c_int32, c_float, c_float, c_float, c_int32, _P, _P,
                                    _P]),
    "ts_tsdf_field": (c_int32, [c_int32, _P, _P, c_int32, _P, _P]),
    "ts_mesh_count_observed": (c_int32, [c_int32, _P, _P, _P, c_float, _P, _P, _P]),
    "ts_mesh_emit_observed": (c_int32, [c_int32, _P, _P, _P, c_float, _P, _P, _P, _P, _P, _P]),
    "ts_field_colors": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P, c_int32, c_int32, _P, _P]),
    "ts_simplify_count": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P]),
    "ts_simplify_keys": (c_int32, [c_int32, _P, _P, _P, _P, _P]),
    "ts_simplify_ws_bytes": (c_int64, [c_int64]),
    "ts_simplify_accumulate": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, c_int32, c_int64, _P, _P, c_int64,
                                         c_int64, _P, _P, _P]),
    "ts_simplify_solve": (c_int32, [c_int32, _P, _P, _P, _P, _P, c_double, _P, _P]),
    "ts_simplify_faces": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P]),
    "ts_clean_degenerate": (c_int32, [c_int32, _P, _P, _P]),
    "ts_clean_edge_keys": (c_int32, [c_int32, c_int32, _P, _P, _P]),
    "ts_clean_face_weights": (c_int32, [c_int32, c_int32, _P, _P, _P, _P]),
    "ts_clean_mark": (c_int32, [c_int32, c_int64, _P, _P, _P, _P]),
    "ts_clean_components": (c_int32, [c_int32, c_int32, _P, _P, _P, _P]),
    "ts_splat_keys": (c_int32, [c_int32, _P, _P, _P, _P]),
    "ts_splat_pack": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_splat_unpack": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_undistort_image": (c_int32, [_P, c_int32, c_int32, POINTER(c_float), POINTER(c_float), POINTER(c_float),
                                     c_int32, c_int32, c_int32, _P, _P]),
    "ts_jpeg_ws_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "ts_jpeg_max_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "ts_jpeg_header": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, _P, c_int64]),
    "ts_jpeg_encode": (c_int32, [_P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, c_int64, _P,
                                 _P, _P]),
    "ts_image_metrics_ws_bytes": (c_int64, [c_int32, c_int32]),
    "ts_image_metrics": (c_int32, [c_int32, c_int32, c_int32, _P, _P, c_int32, _P, _P, _P]),
    "ts_image_metrics_masked_ws_bytes": (c_int64, [c_int32, c_int32]),
    "ts_image_metrics_masked": (c_int32, [c_int32, c_int32, c_int32, _P, _P, c_int32, _P, _P, _P, _P]),
    "ts_depth_prior_project": (c_int32, [c_int32, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_depth_prior_mark": (c_int32, [c_int64, _P, _P, _P]),
    "ts_depth_prior_gather": (c_int32, [c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_depth_prior_fit": (c_int32, [c_int32, _P, _P, _P, _P, c_int32, _P, _P]),
    "ts_depth_prior_apply": (c_int32, [_P, c_int32, c_int32, c_int32, c_int32, _P, c_int32, _P, _P]),
    "ts_label_votes": (c_int32, [c_int32, _CAM, _P, _P, _P, _P, _P, c_int32, _P, _P]),
    "ts_votes_labels": (c_int32, [c_int32, c_int32, _P, c_double, _P, _P, _P]),
    "ts_mcmc_noise": (c_int32, [c_int32, _P, _P, _P, _P, c_float, _P, c_uint64, c_uint32, _P]),
    "ts_mcmc_normals": (c_int32, [c_int32, c_uint64, c_uint32, _P, _P]),
    "ts_mcmc_mean_ws_bytes": (c_int64, [c_int64]),
    "ts_mcmc_mean": (c_int32, [c_int32, c_int64, _P, _P, _P, _P, _P]),
    "ts_mcmc_weights": (c_int32, [c_int32, _P, c_float, c_int32, _P, _P, _P]),
    "ts_mcmc_sample_ws_bytes": (c_int64, [c_int32]),
    "ts_mcmc_sample_rows": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P]),
    "ts_mcmc_rewrite": (c_int32, [c_int32, _P, c_float, _P, _P, c_int32, _P, _P, _P, _P]),
    "ts_mcmc_copy_rows": (c_int32, [c_int32, c_int32, _P, _P, c_int32, _P, _P, _P, _P, _P]),
    "ts_appearance_ws_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "ts_appearance_fwd": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "ts_appearance_bwd": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "ts_grid_tv": (c_int32, [c_int32, c_int32, c_int32, _P, c_float, _P, _P, _P, _P]),
    "ts_affine_fit_ws_bytes": (c_int64, [c_int32, c_int32]),
    "ts_affine_fit_sums": (c_int32, [c_int32, c_int32, _P, _P, c_int32, _P, _P, _P]),
    "ts_transform_gaussians": (c_int32, [c_int32, c_int32, POINTER(c_float), POINTER(c_float), c_float, POINTER(c_float),
                                         _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ts_box_mask": (c_int32, [c_int32, POINTER(c_float), _P, _P, _P]),
    "ts_pose_ws_bytes": (c_int64, [c_int32]),
    "ts_pose_grad": (c_int32, [c_int32, POINTER(c_float), _P, _P, _P, _P, _P, _P, _P]),
    "ts_antialias_fwd": (c_int32, [c_int32, _P, _P, _P, _P, _CAM, c_int32, _P, c_int32, _P, _P, _P, _P]),
    "ts_antialias_bwd": (c_int32, [c_int32, _P, _P, _P, c_int32, _P, _P, _P]),
    "ts_compensation_bwd": (c_int32, [c_int32, _P, _P, _P, _P, _CAM, c_int32, _P, _P, _P, _P, _P]),
}

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Loads the library once; raises HipLibraryError (never falls back) when it is unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise HipLibraryError(
            f"{LIB_PATH} is missing: tinysplat_amd has no CPU or PyTorch fallback. "
            "Build it with `python -m tinysplat_amd._build` (needs hipcc, targets gfx950).")
    stamp = LIB_PATH.with_suffix(LIB_PATH.suffix + ".flags")
    if stamp.exists() and "-DTS_" in stamp.read_text() and os.environ.get("TS_ALLOW_VARIANT_LIB") != "1":
        raise HipLibraryError(
            f"{LIB_PATH} was built with developer -DTS_* overrides (ablation variant; its results may be "
            "wrong). Rebuild with `python -m tinysplat_amd._build`, or set TS_ALLOW_VARIANT_LIB=1.")
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    v = lib.ts_abi_version()
    if v != ABI_VERSION:
        raise HipLibraryError(f"ABI version mismatch: library {v}, binding {ABI_VERSION}")
    if lib.ts_frame_struct_bytes() != ctypes.sizeof(TsFrame):
        raise HipLibraryError("struct ts_frame: the ctypes mirror does not match the library's layout")
    if lib.ts_rank_step_struct_bytes() != ctypes.sizeof(TsRankStep):
        raise HipLibraryError("struct ts_rank_step: the ctypes mirror does not match the library's layout")
    if lib.ts_loss_struct_bytes() != ctypes.sizeof(TsLoss):
        raise HipLibraryError("struct ts_loss: the ctypes mirror does not match the library's layout")
    if lib.ts_tsdf_camera_bytes() != ctypes.sizeof(TsTsdfCamera):
        raise HipLibraryError("struct ts_tsdf_camera: the ctypes mirror does not match the library's layout")
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code == 0:
        return
    if code == -1:
        raise ValueError(f"{what}: bad argument (TS_E_BADARG)")
    if code == -2:
        raise ValueError(f"{what}: SH degree / number of bases not supported (TS_E_DEGREE)")
    raise RuntimeError(f"{what}: HIP error {code}")
