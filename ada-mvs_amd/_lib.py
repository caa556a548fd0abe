"""ctypes binding of libadamvs_hip.so (C ABI: include/adamvs_hip.h).

The library is loaded AFTER `import torch` so that its libamdhip64 dependency
binds to the HIP runtime torch already mapped (one runtime per process).
There is no fallback: if the library is missing or a call fails this raises.
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported before the library is loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADAMVS_LIB_PATH") or os.path.join(_HERE, "libadamvs_hip.so")     # override: A/B of two builds

c_f = ctypes.c_void_p          # device pointer to float
c_i = ctypes.c_int
c_sz = ctypes.c_size_t
c_st = ctypes.c_void_p         # hipStream_t


class FuseWeights(ctypes.Structure):
    """adamvs_fuse_weights"""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "conv1", "gates1", "gates1_b", "cand1", "cand1_b", "conv2", "gates2", "gates2_b",
        "cand2", "cand2_b", "upconv1", "upconv1_b", "final_w", "gates1_w", "gates2_w", "cand2_w", "cand1_w")]


class FConvWeights(ctypes.Structure):
    """adamvs_fconv_weights"""
    _fields_ = [("w", ctypes.c_void_p), ("b", ctypes.c_void_p)]


class ContextWeights(ctypes.Structure):
    """adamvs_context_weights"""
    _fields_ = [("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p)]


class FeatureWeights(ctypes.Structure):
    """adamvs_feature_weights"""
    _fields_ = [(n, FConvWeights) for n in (
        "conv0_0", "conv0_1", "conv1_0", "conv1_1", "conv1_2", "conv2_0", "conv2_1", "conv2_2",
        "out1", "deconv1_t", "deconv1_c", "out2", "deconv2_t", "deconv2_c", "out3")] + \
               [(n, ContextWeights) for n in ("br1_1", "br1_2", "br2_1", "br2_2", "br3_1", "br3_2")]


class FeatureFpnWeights(ctypes.Structure):
    """adamvs_feature_fpn_weights"""
    _fields_ = [(n, FConvWeights) for n in (
        "conv0_0", "conv0_1", "conv1_0", "conv1_1", "conv1_2", "conv2_0", "conv2_1", "conv2_2",
        "out1", "inner1", "out2", "inner2", "out3")]


class StageDesc(ctypes.Structure):
    """adamvs_stage_desc"""
    _fields_ = [(n, ctypes.c_int) for n in ("B", "S", "C", "h", "w", "D", "in_up", "first_stage", "prev_h", "prev_w", "precision", "precision_fuse",
                                            "eps_in_numerator", "plane_mode")] + [("half_span", ctypes.c_float),
                                                                                   ("half_span_dev", ctypes.c_void_p)]


class FusionSource(ctypes.Structure):
    """adamvs_fusion_source"""
    _fields_ = [("depth", ctypes.c_void_p), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("fwd", ctypes.c_float * 12), ("back", ctypes.c_float * 12)]


class DsmGrid(ctypes.Structure):
    """adamvs_dsm_grid"""
    _fields_ = [("x0", ctypes.c_double), ("y_top", ctypes.c_double), ("gsd", ctypes.c_double), ("z_ref", ctypes.c_double),
                ("W", ctypes.c_int), ("H", ctypes.c_int)]


class DsmFillStats(ctypes.Structure):
    """adamvs_dsm_fill_stats"""
    _fields_ = [("cycles", ctypes.c_int), ("converged", ctypes.c_int), ("residual_height", ctypes.c_double),
                ("residual_colour", ctypes.c_double), ("cells_valid", ctypes.c_long), ("cells_filled", ctypes.c_long),
                ("cells_empty", ctypes.c_long)]


class DtmStats(ctypes.Structure):
    """adamvs_dtm_stats"""
    _fields_ = [("levels", ctypes.c_int), ("cells_valid", ctypes.c_long), ("cells_ground", ctypes.c_long),
                ("cells_object", ctypes.c_long), ("cells_empty", ctypes.c_long), ("cells_level", ctypes.c_long * 17)]


class BldStats(ctypes.Structure):
    """adamvs_bld_stats"""
    _fields_ = [("rounds", ctypes.c_int), ("converged", ctypes.c_int), ("tiles", ctypes.c_long), ("pairs", ctypes.c_long),
                ("ms_tile", ctypes.c_float), ("ms_rounds", ctypes.c_float), ("ms_compress", ctypes.c_float)]


class TreeStats(ctypes.Structure):
    """adamvs_tree_stats"""
    _fields_ = [("rounds", ctypes.c_int), ("converged", ctypes.c_int), ("tops", ctypes.c_long), ("candidates", ctypes.c_long),
                ("window_cells", ctypes.c_long), ("ms_parents", ctypes.c_float), ("ms_jump", ctypes.c_float)]


class ContourStats(ctypes.Structure):
    """adamvs_contour_stats"""
    _fields_ = [("rounds", ctypes.c_int), ("rounds_min", ctypes.c_int), ("rounds_dist", ctypes.c_int), ("launched", ctypes.c_int),
                ("converged", ctypes.c_int), ("reserved", ctypes.c_int), ("segments", ctypes.c_long), ("lines", ctypes.c_long),
                ("ms_count", ctypes.c_float), ("ms_rank", ctypes.c_float)]


class DrainStats(ctypes.Structure):
    """adamvs_drain_stats"""
    _fields_ = [("rounds", ctypes.c_int), ("launched", ctypes.c_int), ("converged", ctypes.c_int), ("reserved", ctypes.c_int),
                ("links", ctypes.c_long), ("vertices", ctypes.c_long), ("ms", ctypes.c_float), ("reserved2", ctypes.c_float)]


class SolarStats(ctypes.Structure):
    """adamvs_solar_stats"""
    _fields_ = [("lines", ctypes.c_long), ("spills", ctypes.c_long), ("deepest", ctypes.c_int), ("reserved", ctypes.c_int),
                ("ms", ctypes.c_float), ("reserved2", ctypes.c_float)]


class MeshView(ctypes.Structure):
    """adamvs_mesh_view"""
    _fields_ = [("K", ctypes.c_float * 9), ("R", ctypes.c_float * 9), ("c", ctypes.c_float * 3), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("depth", ctypes.c_void_p), ("rgba", ctypes.c_void_p)]


class MeshBrick(ctypes.Structure):
    """adamvs_mesh_brick"""
    _fields_ = [("origin", ctypes.c_double * 3), ("voxel", ctypes.c_double), ("mu", ctypes.c_double), ("B", ctypes.c_int),
                ("bx", ctypes.c_int), ("by", ctypes.c_int), ("bz", ctypes.c_int), ("min_weight", ctypes.c_int)]


class OrthoGrid(ctypes.Structure):
    """adamvs_ortho_grid"""
    _fields_ = [("x0", ctypes.c_double), ("y_top", ctypes.c_double), ("gsd", ctypes.c_double), ("W", ctypes.c_int), ("H", ctypes.c_int),
                ("K", ctypes.c_int)]


class OrthoView(ctypes.Structure):
    """adamvs_ortho_view"""
    _fields_ = [("C", ctypes.c_double * 3), ("R", ctypes.c_float * 9), ("K", ctypes.c_float * 9), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("rgba", ctypes.c_void_p)]


# name -> (restype, argtypes); every symbol include/adamvs_hip.h declares
SIGNATURES = {
    "adamvs_version": (c_i, []),
    "adamvs_last_error_string": (ctypes.c_char_p, []),
    "adamvs_option_count": (c_i, []),
    "adamvs_option_name": (ctypes.c_char_p, [c_i]),
    "adamvs_option_default": (c_i, [ctypes.c_char_p, ctypes.POINTER(c_i)]),
    "adamvs_get_option": (c_i, [ctypes.c_char_p, ctypes.POINTER(c_i)]),
    "adamvs_set_option": (c_i, [ctypes.c_char_p, c_i]),
    "adamvs_relative_transforms": (c_i, [c_f, c_f, c_i, c_i, c_st]),
    "adamvs_pack_features": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_unpack_features": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_depth_range_samples_uniform": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_depth_range_samples_window": (c_i, [c_f, ctypes.c_double, c_f, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_resize_bilinear": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_depth_regression": (c_i, [c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_homo_warp": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_pair_similarity": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_cost_reg_net_2d_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i]),
    "adamvs_cost_reg_width": (c_i, [c_i, c_i]),
    "adamvs_cost_reg_net_2d_weight_floats": (c_sz, [c_i, c_i]),
    "adamvs_cost_reg_net_2d": (c_i, [c_f, c_f, c_sz, c_f, c_i, c_i, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_conv3x3_dd": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_conv3x3_dd_wino": (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_softmax_max_regress": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_prob_softmax_regress": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_prob_softmax_regress_wino_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "adamvs_prob_softmax_regress_wino": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_conv3x3_dd_wino24": (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_prob_softmax_regress_wino24": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_aggregate_conv1_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i]),
    "adamvs_aggregate_conv1": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_slice_reg_step_scratch_bytes": (c_sz, [c_i, c_i, c_i]),
    "adamvs_slice_reg_step": (c_i, [c_f, c_f, c_f, ctypes.POINTER(FuseWeights), c_f, c_i, c_i, c_i, c_i, c_i, c_i,
                                    ctypes.c_void_p, c_sz, c_st]),
    "adamvs_depth_stage_workspace_bytes": (c_sz, [ctypes.POINTER(StageDesc)]),
    "adamvs_recurrence_schedule": (c_i, [c_i, ctypes.c_longlong]),
    "adamvs_conv_t2_form": (c_i, [c_i, c_i, c_i, c_i]),
    "adamvs_conv_wino24_fold": (c_i, [c_i, c_i, c_i]),
    "adamvs_conv_s2_form": (c_i, [c_i, c_i, c_i, c_i, c_i]),
    "adamvs_conv3x3_dd_wino24_blocks": (c_i, [c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_conv3x3_dd_s2_blocks": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_cost_reg_net_2d_blocks": (c_i, [c_f, c_f, c_sz, c_f, c_i, c_i, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_cost_reg_fold": (c_i, [c_i, c_i, c_i, c_i]),
    "adamvs_gru_wino_mask": (c_i, []),
    "adamvs_depth_stage_forward": (c_i, [ctypes.POINTER(StageDesc), c_f, c_f, c_f, c_f, c_f, c_sz, ctypes.POINTER(FuseWeights),
                                         c_f, c_f, c_f, c_f, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_bench_stage_phase": (c_i, [ctypes.POINTER(StageDesc), c_f, c_f, c_f, c_f, c_f, c_sz, ctypes.POINTER(FuseWeights),
                                       c_f, c_f, c_f, c_f, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_feature_net0_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "adamvs_feature_net0": (c_i, [c_f, ctypes.POINTER(FeatureWeights), c_f, c_f, c_f, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_feature_net0_views": (c_i, [c_f, ctypes.POINTER(FeatureWeights), c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_feature_net_fpn_workspace_bytes": (c_sz, [c_i, c_i, c_i]),
    "adamvs_feature_net_fpn": (c_i, [c_f, ctypes.POINTER(FeatureFpnWeights), c_f, c_f, c_f, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_red_variance_cost": (c_i, [c_f, c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_channel_copy": (c_i, [c_f, c_f, c_i, c_i, c_i, ctypes.c_long, c_i, c_i, ctypes.c_long, c_i, c_i, c_st]),
    "adamvs_group_stats_workspace_bytes": (c_sz, [c_i, c_i]),
    "adamvs_group_stats_partial": (c_i, [c_f, c_f, c_i, c_i, c_i, c_i, ctypes.c_void_p, c_sz, c_st]),
    "adamvs_group_stats_finish": (c_i, [ctypes.c_void_p, c_f, c_i, c_i, c_i, c_i, ctypes.c_float, c_st]),
    "adamvs_gru2_gates_apply": (c_i, [c_f, c_f, c_i, ctypes.c_void_p, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, ctypes.c_float, c_st]),
    "adamvs_conv3x3_pair": (c_i, [c_f, c_i, c_f, c_i, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_gru2_out_apply": (c_i, [c_f, ctypes.c_void_p, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, ctypes.c_float, c_st]),
    "adamvs_red_recur_workspace_bytes": (c_sz, [c_i, c_i, c_i, c_i, c_i, c_i]),
    "adamvs_red_recur_pair": (c_i, [c_f, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_float,
                                    ctypes.c_void_p, c_sz, c_st]),
    "adamvs_red_recur_split": (c_i, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.c_float,
                                     ctypes.c_void_p, c_sz, c_st]),
    "adamvs_soft_argmin": (c_i, [c_f, c_f, c_f, c_f, c_i, c_i, c_i, c_i, c_st]),
    "adamvs_fusion_max_sources": (c_i, []),
    "adamvs_geo_consistency": (c_i, [c_f, c_f, c_i, c_i, ctypes.POINTER(FusionSource), c_i, ctypes.c_float, ctypes.c_float,
                                     ctypes.c_float, c_i, ctypes.c_void_p, c_f, ctypes.c_void_p, c_st]),
    "adamvs_fusion_scan": (c_i, [ctypes.c_void_p, ctypes.c_void_p, c_i, c_st]),
    "adamvs_fusion_emit": (c_i, [c_f, ctypes.c_void_p, c_i, c_i, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_long, c_st]),
    "adamvs_dsm_accumulate": (c_i, [ctypes.POINTER(DsmGrid), ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_i, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_dsm_claim": (c_i, [ctypes.POINTER(DsmGrid), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p,
                               ctypes.c_void_p, c_st]),
    "adamvs_dsm_finalize": (c_i, [ctypes.POINTER(DsmGrid), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i, c_i,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_dsm_fill_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_dsm_fill": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i,
                              ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.POINTER(DsmFillStats), c_st]),
    "adamvs_dtm_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_dsm_open": (c_i, [c_i, c_i, ctypes.c_void_p, c_i, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_dtm_classify": (c_i, [c_i, c_i, ctypes.c_void_p, c_i, ctypes.POINTER(c_i), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p,
                                  ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(DtmStats), c_st]),
    "adamvs_bld_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_bld_flags": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, c_i, c_i, ctypes.c_double, ctypes.c_void_p,
                               ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_bld_label": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.POINTER(BldStats), c_st]),
    "adamvs_bld_table": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_roof_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_roof_links": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                ctypes.c_void_p, c_st]),
    "adamvs_roof_label": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.POINTER(BldStats), c_st]),
    "adamvs_roof_moments": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_long,
                                  ctypes.c_void_p, c_st]),
    "adamvs_roof_grow": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_long, ctypes.c_void_p, ctypes.c_double,
                               c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_roof_residuals": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_long, ctypes.c_void_p,
                                    ctypes.c_double, ctypes.c_void_p, c_st]),
    "adamvs_lod2_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_lod2_corner_heights_host": (c_i, [ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "adamvs_lod2_fill": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_long, c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_lod2_table": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_long, ctypes.c_long,
                                ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_lod2_transpose": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_lod2_count": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                c_st]),
    "adamvs_lod2_runs": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                               ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_tree_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_tree_surface": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, c_i, ctypes.c_void_p, ctypes.c_long,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_tree_parents": (c_i, [c_i, c_i, ctypes.c_void_p, c_i, ctypes.POINTER(c_i), ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                  ctypes.POINTER(TreeStats), c_st]),
    "adamvs_tree_roots": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.POINTER(TreeStats), c_st]),
    "adamvs_tree_crowns": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_long, ctypes.c_void_p,
                                 ctypes.c_void_p, c_st]),
    "adamvs_tree_table": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                c_st]),
    "adamvs_contour_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_contour_rank_workspace_bytes": (ctypes.c_long, [ctypes.c_long]),
    "adamvs_contour_surface": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_double, c_i, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                     ctypes.c_void_p, c_st]),
    "adamvs_contour_count": (c_i, [c_i, c_i, ctypes.c_void_p, c_i, ctypes.POINTER(c_i), ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                   ctypes.POINTER(ContourStats), c_st]),
    "adamvs_contour_segments": (c_i, [c_i, c_i, ctypes.c_void_p, c_i, ctypes.POINTER(c_i), ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_contour_rank": (c_i, [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.POINTER(ContourStats), c_st]),
    "adamvs_contour_lines": (c_i, [c_i, c_i, ctypes.c_void_p, c_i, ctypes.POINTER(c_i), ctypes.c_long, ctypes.c_long] + [ctypes.c_void_p] * 8
                             + [ctypes.c_long] + [ctypes.c_void_p] * 5 + [c_st]),
    "adamvs_drain_workspace_bytes": (ctypes.c_long, [c_i, c_i]),
    "adamvs_drain_fill": (c_i, [c_i, c_i, ctypes.c_void_p, c_i, c_i, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(DrainStats), c_st]),
    "adamvs_drain_direction": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_drain_accumulate": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(DrainStats), c_st]),
    "adamvs_drain_streams": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(DrainStats), c_st]),
    "adamvs_drain_links": (c_i, [c_i, c_i] + [ctypes.c_void_p] * 4 + [ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_long]
                           + [ctypes.c_void_p] * 5 + [c_st]),
    "adamvs_solar_workspace_bytes": (ctypes.c_long, [c_i, c_i, c_i]),
    "adamvs_solar_horizon": (c_i, [c_i, c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.POINTER(SolarStats), c_st]),
    "adamvs_solar_svf": (c_i, [c_i, c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                               ctypes.c_double, ctypes.c_void_p, c_st]),
    "adamvs_solar_expose": (c_i, [c_i, c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.POINTER(c_i),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i), ctypes.POINTER(c_i), ctypes.POINTER(c_i),
                                  ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                  ctypes.c_void_p, c_st]),
    "adamvs_solar_plane_sums": (c_i, [c_i, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, c_st]),
    "adamvs_mesh_check_views": (c_i, [ctypes.POINTER(MeshView), c_i]),
    "adamvs_tsdf_integrate": (c_i, [ctypes.POINTER(MeshBrick), ctypes.c_void_p, c_i, ctypes.c_void_p, c_i, c_f, ctypes.c_void_p,
                                    ctypes.c_void_p, c_st]),
    "adamvs_mesh_classify": (c_i, [ctypes.POINTER(MeshBrick), c_f, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_mesh_count_vertices": (c_i, [ctypes.POINTER(MeshBrick), c_f, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_mesh_emit": (c_i, [ctypes.POINTER(MeshBrick), c_f, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                               ctypes.c_void_p, ctypes.c_long, c_st]),
    "adamvs_simplify_keys": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                   ctypes.c_void_p, c_st]),
    "adamvs_simplify_corners": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, c_i, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, c_st]),
    "adamvs_simplify_accumulate": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_void_p, c_i, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_simplify_solve": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double, ctypes.c_void_p, c_i,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_simplify_solve_host": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "adamvs_simplify_triples": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_simplify_first": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_simplify_mark": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_i, ctypes.c_void_p, c_st]),
    "adamvs_simplify_count": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_simplify_emit": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                   ctypes.c_void_p, ctypes.c_long, c_st]),
    "adamvs_smooth_faces": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_smooth_edge_keys": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_smooth_boundary": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_smooth_filter": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, c_st]),
    "adamvs_smooth_centroids": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_smooth_update": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                   c_st]),
    "adamvs_clean_components": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_clean_area": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_clean_boundary": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_clean_successor": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_clean_double": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_clean_validate": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_i, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_clean_accumulate": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                      ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p,
                                      ctypes.c_void_p, c_st]),
    "adamvs_clean_emit": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_cloud_nearest": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, c_st]),
    "adamvs_cloud_nearest_host": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                        ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "adamvs_cloud_sample_count": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_double, ctypes.c_void_p,
                                        c_st]),
    "adamvs_cloud_sample_emit": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_long, c_st]),
    "adamvs_knn_search": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.c_double, c_i, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long,
                                ctypes.c_longlong, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_knn_search_host": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.c_double, c_i, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "adamvs_knn_normals": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_long, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_knn_normals_host": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_long, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "adamvs_rigid_apply": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                 ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_rigid_apply_host": (c_i, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                      ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]),
    "adamvs_icp_accumulate": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_long, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double, ctypes.c_void_p, c_st]),
    "adamvs_icp_accumulate_host": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_long, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    "adamvs_icp_reduce": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_icp_reduce_host": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]),
    "adamvs_ortho_surface": (c_i, [ctypes.POINTER(OrthoGrid), ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_ortho_zbuf": (c_i, [ctypes.POINTER(OrthoGrid), ctypes.c_void_p, ctypes.POINTER(OrthoView), ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_long, c_st]),
    "adamvs_ortho_compose": (c_i, [ctypes.POINTER(OrthoGrid), ctypes.POINTER(OrthoView), c_i, ctypes.c_void_p, ctypes.c_void_p, c_i,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_ortho_finalize": (c_i, [ctypes.POINTER(OrthoGrid), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_ortho_observe": (c_i, [ctypes.POINTER(OrthoGrid), ctypes.c_void_p, ctypes.POINTER(OrthoView), ctypes.c_void_p, c_i,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_void_p, c_st]),
    "adamvs_ortho_pair_stats": (c_i, [ctypes.c_void_p, c_i, ctypes.c_long, ctypes.c_void_p, c_i, c_i, ctypes.c_void_p, c_st]),
    "adamvs_ortho_adjust_image": (c_i, [ctypes.c_void_p, c_i, c_i, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, c_st]),
    "adamvs_ortho_seam_stats": (c_i, [ctypes.POINTER(OrthoGrid), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_texture_project": (c_i, [ctypes.POINTER(OrthoView), ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_texture_zbuf": (c_i, [ctypes.POINTER(OrthoView), ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_st]),
    "adamvs_texture_score": (c_i, [ctypes.POINTER(OrthoView), c_i, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                   ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, c_st]),
    "adamvs_texture_edge_keys": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_texture_components": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        c_st]),
    "adamvs_texture_rank": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_texture_boxes": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                   ctypes.c_void_p, c_st]),
    "adamvs_texture_fill": (c_i, [ctypes.POINTER(OrthoView), ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_long, c_i, ctypes.c_long,
                                  ctypes.c_void_p, c_st]),
    "adamvs_texture_coords": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_i,
                                    c_i, c_i, c_i, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_texture_level_observe": (c_i, [ctypes.c_void_p, c_i, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, c_st]),
    "adamvs_texture_level_rhs": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                       c_st]),
    "adamvs_texture_level_cg_init": (c_i, [ctypes.c_void_p, ctypes.c_long, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_texture_level_cg": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_double, c_i,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, c_st]),
    "adamvs_texture_level_owner": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, c_i,
                                         ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, c_st]),
    "adamvs_texture_level_dilate": (c_i, [ctypes.c_void_p, ctypes.c_void_p, c_i, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, c_st]),
    "adamvs_texture_level_apply": (c_i, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                         ctypes.c_void_p, c_i, ctypes.c_long, ctypes.c_void_p, c_i, ctypes.c_long, ctypes.c_void_p,
                                         c_st]),
}

ABI_VERSION = 22
PRECISIONS = {"fp32": 0, "bf16x3": 1}
PLANES_EXPLICIT, PLANES_UNIFORM, PLANES_WINDOW = 0, 1, 2
FUSION_TILE = 256                # ADAMVS_FUSION_TILE: pixels per workgroup of the fusion kernels
DSM_MAX, DSM_MEAN = 0, 1         # ADAMVS_DSM_MAX / ADAMVS_DSM_MEAN
DSM_MAX_CELLS = 1 << 28          # ADAMVS_DSM_MAX_CELLS
DSM_FILL_MAX_RADIUS = 1024       # ADAMVS_DSM_FILL_MAX_RADIUS
DTM_MAX_RADIUS = 1024            # ADAMVS_DTM_MAX_RADIUS: largest radius of an opening, cells
DTM_MAX_LEVELS = 16              # ADAMVS_DTM_MAX_LEVELS: most levels of the ground filter
DTM_TILE = 1024                  # ADAMVS_DTM_TILE: cells of a row per workgroup of the running min / max
BLD_TILE_W, BLD_TILE_H = 64, 64  # ADAMVS_BLD_TILE_W / _H: cells of a tile of the component labelling
BLD_MAX_STRIDE = 64              # ADAMVS_BLD_MAX_STRIDE: largest stride of the flatness flag, cells
BLD_MAX_ROUNDS = 64              # ADAMVS_BLD_MAX_ROUNDS: cap on the border rounds of the component labelling
BLD_NOT_CONVERGED = -2           # ADAMVS_BLD_NOT_CONVERGED
BLD_COLUMNS = ("cells", "smooth", "rough", "undetermined", "row_min", "row_max", "col_min", "col_max", "height_sum",
               "height_max_bits")  # ADAMVS_BLD_CELLS .. ADAMVS_BLD_HEIGHT_MAX_BITS: the rows of the component table
ROOF_MAX_SIDE = 32768            # ADAMVS_ROOF_MAX_SIDE: largest W and H of the roof stage, cells
ROOF_MAX_GROW = 256              # ADAMVS_ROOF_MAX_GROW: cap on the growth rounds
ROOF_Q_SCALE, ROOF_Q_MAX = 256, (1 << 19) - 1  # ADAMVS_ROOF_Q_SCALE / _Q_MAX: quantised height above z_ref, 1/256 m
ROOF_COLUMNS = ("n", "su", "sv", "sq", "suu", "suv", "svv", "suq", "svq", "sqq_lo", "sqq_hi", "row_min", "row_max", "col_min", "col_max",
                "q_min", "q_max", "building")  # ADAMVS_ROOF_N .. ADAMVS_ROOF_BUILDING: the rows of the moments table
LOD2_MAX_SIDE = 32768            # ADAMVS_LOD2_MAX_SIDE: largest W and H of the LoD2 stage, cells
LOD2_MAX_FILL = 1024             # ADAMVS_LOD2_MAX_FILL: cap on the fill rounds of the model labels
LOD2_Z_SCALE, LOD2_XY_SCALE = 1024, 1024   # ADAMVS_LOD2_Z_SCALE / _XY_SCALE: heights in 1/1024 m, positions in 1/1024 cell
LOD2_PLANE_BITS = 20             # ADAMVS_LOD2_PLANE_BITS: A, B, C of a plane are multiples of 2^-20 m
LOD2_Z_MAX = 1 << 30             # ADAMVS_LOD2_Z_MAX: |zq| of every corner stays below it
LOD2_BLOCK = 256                 # ADAMVS_LOD2_BLOCK: lattice edges per workgroup of the run kernels
LOD2_COLUMNS = ("cells", "filled", "base", "roof_min")   # ADAMVS_LOD2_CELLS .. ADAMVS_LOD2_ROOF_MIN: the rows of the building table
LOD2_FIELDS = ("orientation", "line", "start", "end", "L", "R", "zL_s", "zL_e", "zR_s",
               "zR_e")           # ADAMVS_LOD2_F_ORIENTATION .. ADAMVS_LOD2_F_ZR_E: the rows of the run records
TREE_TILE = 64                   # ADAMVS_TREE_TILE: cells of a side of a tile of the parents kernel
TREE_MAX_RADIUS = 64             # ADAMVS_TREE_MAX_RADIUS: largest window radius of the local-maximum filter, cells
TREE_MAX_ROUNDS = 32             # ADAMVS_TREE_MAX_ROUNDS: cap on the rounds of pointer jumping
TREE_JUMP_HOPS = 8               # ADAMVS_TREE_JUMP_HOPS: parents followed per cell and round of pointer jumping
TREE_NOT_CONVERGED = -2          # ADAMVS_TREE_NOT_CONVERGED
TREE_Q_SCALE = 256               # ADAMVS_TREE_Q_SCALE: quantised height above ground, 1/256 m
TREE_COLUMNS = ("cells", "q_sum", "q_max", "row_min", "row_max", "col_min", "col_max", "r2_max", "top",
                "s_top")         # ADAMVS_TREE_CELLS .. ADAMVS_TREE_S_TOP: the rows of the tree table
CONTOUR_TILE = 64                # ADAMVS_CONTOUR_TILE: blocks of a side of a tile of the count kernel
CONTOUR_MAX_LEVELS = 4096        # ADAMVS_CONTOUR_MAX_LEVELS: entries of the level table
CONTOUR_MAX_ROUNDS = 64          # ADAMVS_CONTOUR_MAX_ROUNDS: cap on the rounds of list ranking, both phases together
CONTOUR_Q_SCALE = 256            # ADAMVS_CONTOUR_Q_SCALE: quantised height above z_ref, 1/256 m
CONTOUR_MAX_ABS_M = 8191         # ADAMVS_CONTOUR_MAX_ABS_M: |z - z_ref| of a valid cell, metres
CONTOUR_NOT_CONVERGED = -2       # ADAMVS_CONTOUR_NOT_CONVERGED
CONTOUR_TOO_MANY = -3            # ADAMVS_CONTOUR_TOO_MANY
DRAIN_TILE = 32                  # ADAMVS_DRAIN_TILE: cells of a side of a tile of the fill
DRAIN_UNITS = 65536              # ADAMVS_DRAIN_UNITS: units of r and F per metre
DRAIN_NOT_A_FOREST = -2          # ADAMVS_DRAIN_NOT_A_FOREST
SOLAR_STACK_WINDOW = 16          # ADAMVS_SOLAR_STACK_WINDOW: stack entries per line kept in LDS
SOLAR_MAX_SAMPLES = 8192         # ADAMVS_SOLAR_MAX_SAMPLES: rows of the sample table
SOLAR_MAX_SIDE = 32768           # ADAMVS_SOLAR_MAX_SIDE
SOLAR_HEAD_BYTES = 262656        # ADAMVS_SOLAR_HEAD_BYTES: the workspace of the exposure
SOLAR_BAD_LABEL = -2             # ADAMVS_SOLAR_BAD_LABEL
MESH_TILE = 256                  # ADAMVS_MESH_TILE: samples / cubes per workgroup of the mesh kernels
MESH_BRICKS = (32, 64, 128)      # the brick sizes B
MESH_MAX_VIEWS = 65535           # ADAMVS_MESH_MAX_VIEWS
MESH_MAX_EXTENT = 16384.0        # ADAMVS_MESH_MAX_EXTENT, metres from the volume origin
SIMPLIFY_TILE = 256              # ADAMVS_SIMPLIFY_TILE: entries per workgroup of the simplification kernels
SIMPLIFY_KEY_BITS = 21           # ADAMVS_SIMPLIFY_KEY_BITS: bits per axis of a cell key
SMOOTH_TILE = 256                # ADAMVS_SMOOTH_TILE: elements per workgroup of the smoothing kernels
CLEAN_TILE = 256                 # ADAMVS_CLEAN_TILE: elements per workgroup of the cleaning kernels
CLEAN_CHUNK = 1024               # ADAMVS_CLEAN_CHUNK: sorted faces per piece of a component's area
CLEAN_MAX_HOLE_EDGES = 4096      # ADAMVS_CLEAN_MAX_HOLE_EDGES
CLEAN_MAX_ROUNDS = 64            # ADAMVS_CLEAN_MAX_ROUNDS: cap on the rounds of the component labels
CLOUD_TILE = 256                 # ADAMVS_CLOUD_TILE: queries per work item and candidates per tile of the cloud distance
CLOUD_MAX_SUBDIV = 1024          # ADAMVS_CLOUD_MAX_SUBDIV: largest n of a face of the surface sampler
KNN_MAX_K = 32                   # ADAMVS_KNN_MAX_K: largest k of the cloud neighbourhoods
KNN_RANK_EPS = 1e-12             # ADAMVS_KNN_RANK_EPS: a neighbourhood with lambda1 <= eps lambda2 is collinear
KNN_VALID, KNN_TOO_FEW, KNN_COLLINEAR = 0, 1, 2    # ADAMVS_KNN_VALID / _TOO_FEW / _COLLINEAR: the flag of a normal
ICP_TERMS = 32                   # ADAMVS_ICP_TERMS: sums of one accumulation of the cloud registration
ORTHO_BEST, ORTHO_FEATHER = 0, 1 # ADAMVS_ORTHO_BEST / ADAMVS_ORTHO_FEATHER
ORTHO_MAX_CELLS = 1 << 28        # ADAMVS_ORTHO_MAX_CELLS
ORTHO_MAX_UPSAMPLE = 8           # ADAMVS_ORTHO_MAX_UPSAMPLE
ORTHO_BAL_MAX_SAMPLES = 1 << 20  # ADAMVS_ORTHO_BAL_MAX_SAMPLES: most cells of the balance's observation lattice
ORTHO_BAL_CHUNK = 8192           # ADAMVS_ORTHO_BAL_CHUNK: lattice cells per workgroup of the pair statistics
ORTHO_BAL_MAX_Q = 16320          # ADAMVS_ORTHO_BAL_MAX_Q: 64 x 255, the largest quantised colour
TEXTURE_TILE = 256               # ADAMVS_TEXTURE_TILE: faces per workgroup of the texture kernels
TEXTURE_PAGES = (1024, 16384)    # ADAMVS_TEXTURE_MIN_PAGE, ADAMVS_TEXTURE_MAX_PAGE
TEXTURE_MAX_FACES = (1 << 31) - 1 # ADAMVS_TEXTURE_MAX_FACES
TEXTURE_LEVEL_MAX_NODES = 1 << 30 # ADAMVS_TEXTURE_LEVEL_MAX_NODES
TEXTURE_LEVEL_BLOCKS = 2048    # ADAMVS_TEXTURE_LEVEL_BLOCKS: workgroups (and partial sums) of a dot product of the seam solve
TEXTURE_LEVEL_BAND = 2           # ADAMVS_TEXTURE_LEVEL_BAND: dilation rounds of the owner map
PHASE_VIEW_WEIGHTS, PHASE_AGGREGATE, PHASE_RECURRENCE, PHASE_SOFT_ARGMIN, PHASE_ALL = 1, 2, 4, 8, 15
_lib = None


class AdaMVSHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes library; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdaMVSHipError(
            "libadamvs_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "-- there is no CPU fallback for the Ada-MVS hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    v = lib.adamvs_version()
    if v != ABI_VERSION:
        raise AdaMVSHipError("libadamvs_hip.so ABI version %d, host expects %d: rebuild" % (v, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    """Map the C status code to an exception (0 ok, <0 argument error, >0 hipError_t)."""
    if rc == 0:
        return
    msg = load().adamvs_last_error_string().decode("utf-8", "replace")
    kind = "invalid argument" if rc < 0 else "HIP error %d" % rc
    raise AdaMVSHipError("%s failed (%s): %s" % (what, kind, msg))


def set_option(name, value):
    """adamvs_set_option: one of the integers of include/adamvs_hip.h "OPTIONS" (which of two equivalent kernel forms a layer takes)."""
    check(load().adamvs_set_option(name.encode(), int(value)), "adamvs_set_option(%s)" % name)


def get_option(name):
    v = c_i(0)
    check(load().adamvs_get_option(name.encode(), ctypes.byref(v)), "adamvs_get_option(%s)" % name)
    return v.value


def option_names():
    lib = load()
    return [lib.adamvs_option_name(i).decode() for i in range(lib.adamvs_option_count())]


class options:
    """`with _lib.options(winograd=0, gru_wino=0): ...` -- set for the block, restored afterwards (tests, A/B timing)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            set_option(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.saved.items():
            set_option(k, v)
