"""ctypes binding of the C ABI declared in include/pda_pointnet2.h and include/pda_train.h.

The library is the product: if it is missing or a symbol is absent this module raises at
import of the first op -- there is no fallback path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PDA_LIB_PATH: load another build of the same ABI (A/B timing of kernel variants)
LIB_PATH = os.environ.get("PDA_LIB_PATH") or os.path.join(_HERE, "libpda_pointnet2.so")
ABI_VERSION = 20


class DensityNetScale(ctypes.Structure):
    """pda_densitynet_scale_t (include/pda_train.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("grad_y", ctypes.c_void_p), ("params", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("stats", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("running", ctypes.c_void_p * 6),
                ("grad_params", ctypes.c_void_p), ("n", ctypes.c_int64), ("rowmap", ctypes.c_void_p),
                ("row_weight", ctypes.c_void_p), ("n_unique", ctypes.c_void_p), ("nsample", ctypes.c_int),
                ("eps", ctypes.c_float), ("momentum", ctypes.c_float)]


class OnceFrames(ctypes.Structure):
    """pda_once_frames_t (include/pda_train.h)."""
    _fields_ = [("gt_boxes", ctypes.c_void_p), ("gt_name", ctypes.c_void_p), ("gt_offsets", ctypes.c_void_p),
                ("pred_boxes", ctypes.c_void_p), ("pred_score", ctypes.c_void_p), ("pred_name", ctypes.c_void_p),
                ("pred_start", ctypes.c_void_p), ("pred_count", ctypes.c_void_p), ("iou_start", ctypes.c_void_p),
                ("n_gt_total", ctypes.c_int64), ("pred_cap", ctypes.c_int64), ("iou_cap", ctypes.c_int64),
                ("n_frames", ctypes.c_int), ("max_gt", ctypes.c_int), ("max_pred", ctypes.c_int)]


class KittiFrames(ctypes.Structure):
    """pda_kitti_frames_t (include/pda_train.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("gt_bbox", "gt_loc", "gt_dims", "gt_ry", "gt_alpha", "gt_trunc", "gt_occ",
                                               "gt_name", "gt_offsets", "dt_bbox", "dt_box", "dt_alpha", "dt_score",
                                               "dt_name", "dt_start", "dt_count", "ov_start", "frame_mode")] + \
               [("n_gt_total", ctypes.c_int64), ("det_cap", ctypes.c_int64), ("ov_cap", ctypes.c_int64),
                ("n_frames", ctypes.c_int), ("max_gt", ctypes.c_int), ("max_det", ctypes.c_int)]


class ParamGradEntry(ctypes.Structure):
    """pda_param_grad_entry_t (include/pda_train.h)."""
    _fields_ = [("kind", ctypes.c_int32), ("count", ctypes.c_int32), ("part", ctypes.c_void_p), ("part_bias", ctypes.c_void_p),
                ("dst", ctypes.c_void_p), ("dst_bias", ctypes.c_void_p), ("nm", ctypes.c_int64), ("n", ctypes.c_int32),
                ("cols", ctypes.c_int32), ("ld", ctypes.c_int64)]


# The two epochs of param_cache.py (which explains them and owns every read and write inside the package).
PARAM_EPOCH = [0]
WEIGHT_EPOCH = [0]

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float

# name -> argtypes, in the order of include/pda_pointnet2.h
SIGNATURES = {
    "pda_furthest_point_sampling": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "pda_furthest_point_sampling_with_dist": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "pda_gather_points": [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "pda_gather_points_grad": [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "pda_ball_query": [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp],
    "pda_ball_query_dilated": [_vp, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp],
    "pda_ellipsoid_query": [_vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _i, _vp],
    "pda_ball_query_cells_scratch_bytes": [_i, _i],
    "pda_ball_query_cells": [_vp, _vp, ctypes.POINTER(_vp), _i, _i, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_int32),
                             _vp, ctypes.c_int64, _vp],
    "pda_ball_query_multi": [_vp, _vp, ctypes.POINTER(_vp), _i, _i, _i, _i,
                             ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_int32), _vp],
    "pda_group_points": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_group_points_grad": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_group_rows": [_vp, _vp, _vp, _i, _i, _i, ctypes.c_int64, _vp],
    "pda_group_rows_grad": [_vp, _vp, _vp, _i, _i, _i, ctypes.c_int64, _vp],
    "pda_three_nn": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "pda_three_interpolate": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "pda_three_interpolate_grad": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "pda_chamfer_forward": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "pda_chamfer_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "pda_group_attention_fwd": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_group_attention_bwd": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_group_attention_fwd_bf16": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_group_attention_bwd_bf16": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_sa_mlp_maxpool": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32),
                           ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp],
    "pda_linear_cols_packed_size": [_i, _i],
    "pda_linear_cols_pack": [_vp, _vp, _i, _i, _i, _i, _vp],
    "pda_linear_cols": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],
    "pda_sa_gather_linear": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "pda_linear_split_packed_bytes": [_i, _i],
    "pda_linear_split_pack": [_vp, _vp, _i, _i, _i, _vp],
    "pda_linear_split_pack_both": [_vp, _vp, _vp, _i, _i, _vp],
    "pda_linear_split": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_gemm_split": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _i, _vp],
    "pda_sa_mlp_packed_size": [_i, _i, _i],
    "pda_sa_mlp_pack_weights": [_vp, _vp, _i, _i, _i, _vp],
    # include/pda_train.h
    "pda_grad_norm": [_vp, ctypes.c_int64, _vp, _vp, _vp],
    "pda_bn_relu_scratch_bytes": [_i],
    "pda_bn_relu_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _f, _f, _vp],
    "pda_bn_relu_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp],    "pda_bn_relu_fwd_mixed": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, ctypes.c_int64, _i, _f, _f, _vp],
    "pda_bn_relu_bwd_mixed": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp],
    "pda_bn_relu_max_pool_fwd": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _f, _f, _vp],
    "pda_bn_relu_max_pool_bwd": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],

    "pda_layer_norm_scratch_bytes": [_i],
    "pda_layer_norm_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _f, _vp],
    "pda_layer_norm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp],
    "pda_layer_norm_fwd_mixed": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _f, _vp],
    "pda_layer_norm_bwd_mixed": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp],
    "pda_linear_wgrad_scratch_bytes": [ctypes.c_int64, _i, _i],
    "pda_linear_wgrad_form": [ctypes.c_int64, _i, _i],
    "pda_linear_wgrad": [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],
    "pda_linear_wgrad_bn": [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp, _vp, _vp, _vp],
    "pda_linear_wgrad_partials": [_vp, _vp, _vp, _i, ctypes.c_int64, _i, _i, ctypes.POINTER(_i), _vp],
    "pda_linear_wgrad_bn_partials": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp, _vp, _vp, ctypes.POINTER(_i), _vp],
    "pda_layer_norm_bwd_partials": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, ctypes.POINTER(_i), _vp],
    "pda_param_grad_reduce_grouped": [ctypes.POINTER(ParamGradEntry), _i, _vp],
    "pda_gemm_split_bn_tiles": [ctypes.c_int64],
    "pda_gemm_split_bn": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "pda_gemm_split_maxpool": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _i, _vp],
    "pda_gemm_split_gather": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "pda_bn_stats_fwd": [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _f, _f, _vp],
    "pda_bn_finalize_fwd": [_vp, _i, _i, ctypes.c_int64, _f, _f, _vp, _vp, _vp, _vp],
    "pda_bn_relu_max_pool_apply": [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],
    "pda_bn_relu_bwd_reduce": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp],
    "pda_colsum_scratch_bytes": [_i],
    "pda_colsum_bf16": [_vp, _vp, _vp, ctypes.c_int64, _i, _vp],
    "pda_assemble_tokens": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_assemble_tokens_grad": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_add_max_pool": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],
    "pda_max_pool_scatter": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],
    "pda_add_max_pool_bf16": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],
    "pda_max_pool_scatter_bf16": [_vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _vp],
    "pda_ragged_plan": [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp],
    "pda_assemble_tokens_ragged": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _i, _i, _i, _vp],
    "pda_assemble_tokens_ragged_grad": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _i, _i, _i, _vp],
    "pda_bn_relu_fwd_weighted": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _f, _f, _vp, ctypes.c_int64, _vp],
    "pda_bn_relu_bwd_weighted": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp, ctypes.c_int64, _vp],
    "pda_add_max_pool_ragged": [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp],
    "pda_max_pool_scatter_ragged": [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _vp],
    "pda_group_attention_ragged_fwd": [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_group_attention_ragged_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_densitynet_param_count": [],
    "pda_densitynet_eval_param_count": [],
    "pda_densitynet_scratch_bytes": [],
    "pda_densitynet_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _f, _f, _vp],
    "pda_densitynet_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _f, _vp],
    "pda_densitynet_eval": [_vp, _vp, _vp, ctypes.c_int64, _vp],
    "pda_densitynet_fwd_multi": [_vp, _i, _vp],
    "pda_densitynet_bwd_multi": [_vp, _i, _vp],
    "pda_densitynet_fwd_unique": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _i, _f, _f, _vp],
    "pda_densitynet_bwd_unique": [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _i, _f, _vp],
    "pda_pda_geometry": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp],
    "pda_points_in_boxes": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "pda_roiaware_pool3d_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "pda_roiaware_pool3d_bwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "pda_roipoint_pool3d_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_points_in_boxes_mask": [_vp, _vp, _vp, _i, _i, _vp],
    "pda_points_in_boxes_count": [_vp, _i, _vp, _vp, _i, _i, _i, _vp],
    "pda_assign_point_targets": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_sa_gaussian_mask": [_vp, _i, _i, _vp, _vp, _vp, ctypes.c_int64, _vp],
    "pda_head_assign_targets": [_vp, _i, _i, _vp, ctypes.POINTER(ctypes.c_float), _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "pda_head_cls_loss": [_vp, _i, _i, _i, _vp, _vp, ctypes.c_int64, _f, _vp, _vp, _vp],
    "pda_head_centerness": [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp],
    "pda_head_box_loss": [_vp, _vp, _vp, _vp, _f, _i, _f, _f, ctypes.c_int64, _vp, _vp, _vp],
    "pda_head_vote_loss": [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, ctypes.c_int64, _vp, _vp, _vp],
    "pda_head_corner_loss": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _f, ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_boxes_overlap_bev": [_vp, _vp, _vp, _i, _i, _vp],
    "pda_boxes_iou_bev": [_vp, _vp, _vp, _i, _i, _vp],
    "pda_nms_mask_words": [_i],
    "pda_nms_bev": [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp],
    "pda_sa_small_train_workspace_bytes": [],
    "pda_sa_small_train_supported": [_i, _i, _i, _i, _i, ctypes.c_int64],
    "pda_sa_small_train_fwd": [_vp] * 7 + [ctypes.POINTER(_vp)] * 4 + [ctypes.POINTER(_f)] * 2 + [_vp] * 4 + [_i] * 8 + [_vp],
    "pda_sa_small_train_bwd": [_vp] * 13 + [ctypes.POINTER(_vp)] * 2 + [_i] * 8 + [_vp],
    "pda_sa_xyz_grad_scratch_bytes": [_i],
    "pda_sa_point_gather": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_sa_xyz_grad": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_sa_point_gather_stats_blocks": [ctypes.c_int64, _i],
    "pda_sa_point_gather_stats": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_sa_point_grad_bn": [_vp] * 10 + [_i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_adam_onecycle_step": [_vp, _vp, _vp, _vp, ctypes.c_int64, _f, _f, _f, _f, _f, _i, _vp, _f, _vp],
    "pda_input_stage_workspace_bytes": [_i, ctypes.c_int64],
    "pda_input_stage": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, ctypes.POINTER(_f), _i, _vp, _vp, _vp,
                        ctypes.c_uint64, _i, _vp, _vp, _vp, _vp],
    "pda_input_boxes": [_vp, _vp, ctypes.c_int64, _i, _i, _i, ctypes.POINTER(_f), _i, _vp, _vp, _vp],
    "pda_augment_workspace_bytes": [_i, ctypes.c_int64, _i],
    "pda_augment": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp,
                    _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, ctypes.POINTER(_f), ctypes.c_int64, _vp, ctypes.c_int64,
                    _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_augment_paste": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp,
                          _vp, _vp, _i, _vp, _vp, _vp, _i, ctypes.POINTER(_f), ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp,
                          ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_augment_steps_workspace_bytes": [_i, ctypes.c_int64, _i, _i],
    "pda_augment_steps": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, ctypes.c_int64,
                          ctypes.POINTER(ctypes.c_int32), _i, _vp, _vp, _i, _i, _vp, _vp, ctypes.c_int64, _vp, _vp,
                          ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_pyramid_aug_workspace_bytes": [_i, ctypes.c_int64, _i],
    "pda_pyramid_aug": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _i,
                        ctypes.POINTER(ctypes.c_double), _i, _i, _i, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp,
                        _vp, _vp, _vp],
    "pda_once_eval_workspace_bytes": [_i, ctypes.c_int64, _i],
    "pda_once_eval_iou": [ctypes.POINTER(OnceFrames), _i, _vp, _vp, _vp],
    "pda_once_eval_accumulate": [ctypes.POINTER(OnceFrames), _vp, _vp, _i, _i, ctypes.POINTER(ctypes.c_double), _i, _vp, _vp,
                                 _vp, _vp],
    "pda_once_eval_match": [ctypes.POINTER(OnceFrames), _vp, _vp, _i, _i, ctypes.POINTER(ctypes.c_double), _i, _i, _vp, _vp,
                            _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_kitti_eval_workspace_bytes": [_i, ctypes.c_int64, ctypes.c_int64, _i],
    "pda_kitti_eval_overlaps": [ctypes.POINTER(KittiFrames), _vp, _vp, _vp],
    "pda_kitti_eval_first_pass": [ctypes.POINTER(KittiFrames), _vp, _i, _i, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_double),
                                  _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_kitti_eval_match": [ctypes.POINTER(KittiFrames), _vp, _i, _i, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_double), _i,
                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_kitti_eval_predictions": [_vp, ctypes.c_int64, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "pda_recall_record": [_vp, _vp, _vp, _i, ctypes.POINTER(_f), _i, _vp, _vp, _i, _i, _i, _vp],
    "pda_roi_max_iou": [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp],
    "pda_roi_sample_targets": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i] + [ctypes.c_double] * 5 + [_i, _vp, _vp, _vp, _vp,
                               ctypes.c_uint64] + [_vp] * 10 + [_i, _i, _i, _vp],
    "pda_kitti_fov_filter_workspace_bytes": [_i, ctypes.c_int64],
    "pda_kitti_fov_filter": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_gt_extract_workspace_bytes": [_i, ctypes.c_int64, ctypes.c_int64],
    "pda_gt_extract_count": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_gt_extract_write": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp,
                             ctypes.c_int64, _vp, _vp, _vp],
    "pda_voxel_workspace_bytes": [_i, ctypes.c_int64, _i, _i],
    "pda_voxelize": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, ctypes.POINTER(_f), ctypes.POINTER(_f),
                     ctypes.POINTER(ctypes.c_int32), _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_voxel_sample": [_vp, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, ctypes.POINTER(_f), ctypes.POINTER(_f),
                         ctypes.POINTER(ctypes.c_int32), _i, _i, _i, _i, _i, _vp, _vp, ctypes.c_int64, ctypes.c_uint64, _vp,
                         ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_dyn_voxel_workspace_bytes": [ctypes.c_int64, _i],
    "pda_dyn_voxel_index": [_vp, ctypes.c_int64, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_int32),
                            _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_dyn_scatter_mean": [_vp, _i, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp],
    "pda_dyn_scatter_max_fwd": [_vp, _i, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp],
    "pda_dyn_scatter_max_bwd": [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _vp, _vp],
    "pda_dyn_pillar_features": [_vp, ctypes.c_int64, _i, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_f), ctypes.POINTER(_f), _i,
                                _i, _vp, _vp],
    "pda_pillar_scatter_fwd": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _i, _vp, _vp],
    "pda_pillar_scatter_bwd": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, _i, _i, _vp, _vp],
    "pda_center_assign_targets": [_vp, _i, _i, _i, _i, _i] + [ctypes.POINTER(ctypes.c_int32)] * 3 + [_i, _i, _i]
                                 + [ctypes.c_double] * 6 + [_i] + [ctypes.POINTER(_vp)] * 4 + [_vp],
    "pda_center_focal_blocks": [ctypes.c_int64],
    "pda_center_focal_loss": [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp],
    "pda_center_scale": [_vp, _vp, _vp, _f, ctypes.c_int64, _vp, _vp],
    "pda_center_reg_loss": [ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_int32), _i, _vp, _vp, _vp, ctypes.POINTER(_f), _f, _i,
                            _i, ctypes.c_int64, _vp, _vp],
    "pda_center_reg_loss_grad": [ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_int32), _i, _vp, _vp, _vp, ctypes.POINTER(_f), _f,
                                 _i, _i, ctypes.c_int64, _vp, _vp, ctypes.POINTER(_vp), _vp],
    "pda_center_decode": [_vp] * 7 + [_i] * 5 + [ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_double] * 5
                         + [ctypes.POINTER(_f), _i, ctypes.c_double, _vp, _vp, _vp, _vp],
    "pda_anchor_assign_targets": [_vp, _i, _i, _i, _vp, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_f),
                                  ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_anchor_loss_blocks": [ctypes.c_int64],
    "pda_anchor_loss": [_vp] * 7 + [_i] * 4 + [ctypes.POINTER(_f)] + [ctypes.c_double] * 4 + [_vp] * 6,
    "pda_anchor_decode": [_vp, _vp, _vp, _i, _i, _i, ctypes.c_double, ctypes.c_double, _vp, _vp],
    "pda_anchor_multi_assign_targets": [_vp, _i, _i, _i, _vp, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_f),
                                        ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_anchor_multi_loss_blocks": [ctypes.c_int64],
    "pda_anchor_multi_loss": [ctypes.POINTER(_vp)] * 3 + [_i] + [ctypes.POINTER(ctypes.c_int32)] * 3 + [_vp] * 4 + [_i] * 4
                             + [ctypes.POINTER(_f)] + [ctypes.c_double] * 6 + [ctypes.POINTER(_vp)] * 3 + [_vp] * 3,
    "pda_multi_nms_compact": [_vp] * 5 + [_i] * 4 + [_vp] * 5,
    "pda_anchor_assign_targets_coded": [_vp, _i, _i, _i, _i, _vp, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_f),
                                        ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_anchor_multi_assign_targets_coded": [_vp, _i, _i, _i, _i, _vp, _i, _i, ctypes.POINTER(ctypes.c_int32),
                                              ctypes.POINTER(_f), ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp,
                                              _vp, _vp, _vp],
    "pda_anchor_loss_coded": [_i] * 3 + [_vp] * 7 + [_i] * 4 + [ctypes.POINTER(_f)] + [ctypes.c_double] * 4 + [_vp] * 6,
    "pda_anchor_decode_coded": [_i, _i, _vp, _vp, _vp, _i, _i, _i, ctypes.c_double, ctypes.c_double, _vp, _vp],
    "pda_anchor_multi_loss_coded": [_i] * 3 + [ctypes.POINTER(_vp)] * 3 + [_i] + [ctypes.POINTER(ctypes.c_int32)] * 3 + [_vp] * 4
                                   + [_i] * 4 + [ctypes.POINTER(_f)] + [ctypes.c_double] * 6 + [ctypes.POINTER(_vp)] * 3 + [_vp] * 3,
    "pda_multi_nms_compact_wide": [_i] + [_vp] * 5 + [_i] * 4 + [_vp] * 5,
    "pda_pillar_features": [_vp, _vp, _vp, ctypes.c_int64, _i, _i, ctypes.POINTER(_f), ctypes.POINTER(_f), _i, _i, _vp, _vp],
    "pda_spconv_index_workspace_bytes": [ctypes.c_int64, ctypes.c_int64, _i],
    "pda_spconv_index_subm": [_vp, ctypes.c_int64] + [_i] * 7 + [_vp, _vp, _vp, _vp],
    "pda_spconv_index_strided": [_vp, ctypes.c_int64] + [_i] * 13 + [ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp],
    "pda_spconv_index_subm_counted": [_vp, ctypes.c_int64, _vp] + [_i] * 7 + [_vp, _vp, _vp, _vp],
    "pda_spconv_index_strided_counted": [_vp, ctypes.c_int64, _vp] + [_i] * 13 + [ctypes.c_int64] + [_vp] * 7,
    "pda_bn_relu_fwd_counted": [_vp] * 8 + [ctypes.c_int64, _i, _f, _f, _vp, _vp, _i, _i, _vp],
    "pda_bn_relu_bwd_counted": [_vp] * 9 + [ctypes.c_int64, _i, _vp, _i, _i, _vp],
    "pda_bn_add_relu_fwd_counted": [_vp] * 9 + [ctypes.c_int64, _i, _f, _f, _vp, _vp, _i, _vp],
    "pda_bn_add_relu_bwd_counted": [_vp] * 11 + [ctypes.c_int64, _i, _vp, _i, _vp],
    "pda_spconv_gemm": [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _i, _i, _i, _vp],
    "pda_spconv_wgrad_workspace_bytes": [ctypes.c_int64, _i, _i, _i],
    "pda_spconv_wgrad": [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _i, _vp, _vp, _vp, _vp],
    "pda_voxel_pool_scratch_doubles": [_i, _i, _i],
    "pda_voxel_pool_moments": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "pda_voxel_pool_fwd": [_vp] * 9 + [_i, _i, _i, _i, _vp],
    "pda_voxel_pool_bwd": [_vp] * 10 + [_i, _i, _i, _i, _vp],
    "pda_stack_sa_scratch_doubles": [_i, _i, _i, _i],
    "pda_stack_sa_moments": [_vp] * 9 + [_i] * 5 + [_vp],
    "pda_stack_sa_fwd": [_vp] * 15 + [_i] * 6 + [_vp],
    "pda_stack_sa_apply": [_vp, _vp, _vp, _vp, _i, _i, _vp],
    "pda_stack_sa_bwd1": [_vp] * 18 + [_i] * 6 + [_vp],
    "pda_stack_sa_bwd2": [_vp] * 14 + [_i] * 5 + [_vp],
    "pda_bev_interpolate_fwd": [_vp] * 5 + [_i] * 5 + [_vp],
    "pda_bev_interpolate_bwd": [_vp] * 5 + [_i] * 5 + [_vp],
    "pda_bev_roi_grid_pool": [_vp] * 3 + [_i] * 6 + [_f] * 4 + [_vp],
    "pda_roipoint_pool3d_canonical_fwd": [_vp] * 4 + [ctypes.POINTER(_f), _f, _vp, _vp] + [_i] * 5 + [_vp],
    "pda_part_assign_targets": [_vp, _vp, ctypes.POINTER(_f), _vp, _vp, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_part_loss_blocks": [ctypes.c_int64],
    "pda_part_loss": [_vp, _vp, _vp, ctypes.c_double, _vp, _vp, _vp, ctypes.c_int64, _vp],
    "pda_parta2_pool_workspace_bytes": [ctypes.c_int64, _i],
    "pda_parta2_pool_segments": [_vp, ctypes.c_int64, _i, _vp, _vp, _vp],
    "pda_parta2_pool_collect": [_vp, _vp, _vp, _vp, _i, _i, ctypes.c_int64, _i, _i, _vp],
    "pda_parta2_pool_sparsify": [_vp, _vp, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _vp],
    "pda_parta2_pool_features": [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _i, _vp],
    "pda_parta2_pool_bwd": [_vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _vp],
    "pda_roi_point_filter": [_vp, _vp, _vp, _f, _vp, _vp, ctypes.c_int64, _i, _i, _i, _i, _vp],
    "pda_vector_interp_fwd": [_vp] * 6 + [_i] * 4 + [_vp],
    "pda_vector_interp_bwd": [_vp] * 4 + [_i] * 4 + [_vp],
    "pda_frustum_sample_fwd": [_vp] * 6 + [_i] * 8 + [ctypes.POINTER(_f)] * 2 + [_i, _f, _f, _vp],
    "pda_frustum_sample_bwd": [_vp] * 8 + [_i] * 8 + [ctypes.POINTER(_f)] * 2 + [_i, _f, _f, _vp],
    "pda_ddn_loss_blocks": [ctypes.c_int64],
    "pda_ddn_loss_fwd_bwd": [_vp] * 6 + [_i] * 6 + [_f] * 3 + [ctypes.c_double] * 5 + [_vp],
    # include/pda_pointnet2_stack.h
    "pda_stack_ball_query": [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp],
    "pda_stack_group_points": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "pda_stack_group_points_grad": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "pda_stack_furthest_point_sampling": [_vp, _vp, _vp, _vp, _vp, _i, _vp],
    "pda_stack_three_nn": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "pda_stack_three_interpolate": [_vp, _vp, _vp, _vp, _i, _i, _vp],
    "pda_stack_three_interpolate_grad": [_vp, _vp, _vp, _vp, _i, _i, _vp],
    "pda_stack_voxel_query": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp],
    "pda_stack_query_local_neighbor_idxs": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _i, _i, _i, _i, _vp],
    "pda_stack_three_nn_by_local_idxs": [_vp, _vp, _vp, _vp, _vp, _vp, _i, ctypes.c_int64, _i, _i, _vp],
    "pda_stack_vector_pool": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i,
                              _i, _i, _i, _vp],
    "pda_stack_vector_pool_grad": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
}
# the entries of SIGNATURES that return a size (int64_t) where every other one returns a status (int)
SIZE_QUERIES = [
    "pda_nms_mask_words", "pda_ball_query_cells_scratch_bytes", "pda_bn_relu_scratch_bytes",
    "pda_layer_norm_scratch_bytes", "pda_linear_wgrad_scratch_bytes", "pda_linear_split_packed_bytes",
    "pda_colsum_scratch_bytes", "pda_gemm_split_bn_tiles", "pda_densitynet_scratch_bytes",
    "pda_sa_small_train_workspace_bytes", "pda_sa_xyz_grad_scratch_bytes", "pda_sa_point_gather_stats_blocks",
    "pda_input_stage_workspace_bytes",
    "pda_augment_workspace_bytes", "pda_augment_steps_workspace_bytes", "pda_pyramid_aug_workspace_bytes",
    "pda_once_eval_workspace_bytes",
    "pda_kitti_eval_workspace_bytes", "pda_kitti_fov_filter_workspace_bytes", "pda_gt_extract_workspace_bytes",
    "pda_voxel_workspace_bytes", "pda_dyn_voxel_workspace_bytes", "pda_center_focal_blocks", "pda_anchor_loss_blocks",
    "pda_anchor_multi_loss_blocks",
    "pda_spconv_index_workspace_bytes", "pda_spconv_wgrad_workspace_bytes", "pda_voxel_pool_scratch_doubles",
    "pda_stack_sa_scratch_doubles", "pda_part_loss_blocks", "pda_parta2_pool_workspace_bytes", "pda_ddn_loss_blocks"]
INFO_SYMBOLS = ["pda_abi_version", "pda_last_error", "pda_fp_contract_mode", "pda_opt_n_threads",
                "pda_fps_coop_timeouts", "pda_debug_fps_spin_limit", "pda_debug_fps_exchange_nonzero"]

_LIB = None


class PdaError(RuntimeError):
    pass


def load():
    """Load libpda_pointnet2.so (after torch, so both share one HIP runtime)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  (loads libamdhip64 first; our NEEDED soname resolves to it)
    if not os.path.exists(LIB_PATH):
        raise PdaError(
            "%s not found: build it with `python -m pdanet_amd.build` (hipcc, gfx950). "
            "pdanet_amd has no fallback path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.argtypes = argtypes
        fn.restype = _i
    for name in SIZE_QUERIES:
        getattr(lib, name).restype = ctypes.c_int64
    lib.pda_abi_version.restype = _i
    lib.pda_last_error.restype = ctypes.c_char_p
    lib.pda_fp_contract_mode.restype = _i
    lib.pda_opt_n_threads.argtypes = [_i]
    lib.pda_opt_n_threads.restype = _i
    lib.pda_fps_coop_timeouts.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), _i]
    lib.pda_fps_coop_timeouts.restype = _i
    lib.pda_debug_fps_spin_limit.argtypes = [_i]
    lib.pda_debug_fps_spin_limit.restype = _i
    lib.pda_debug_fps_exchange_nonzero.argtypes = []
    lib.pda_debug_fps_exchange_nonzero.restype = ctypes.c_longlong
    if lib.pda_abi_version() != ABI_VERSION:
        raise PdaError("libpda_pointnet2.so ABI %d != binding ABI %d: rebuild"
                       % (lib.pda_abi_version(), ABI_VERSION))
    _LIB = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().pda_last_error().decode("utf-8", "replace")
        raise PdaError("%s failed with status %d: %s" % (what, status, msg))
