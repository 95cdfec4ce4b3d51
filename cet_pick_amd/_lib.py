"""ctypes binding of the C-ABI in include/cetpick_hip.h.

The product path has no CPU fallback: if libcetpick_hip.so is missing or a call fails this module
raises.  PyTorch is only the owner of device memory and streams here.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CETPICK_HIP_LIB") or os.path.join(_HERE, "libcetpick_hip.so")   # env: tuning builds

_c = ctypes
_P, _I, _F, _Z, _D, _L = _c.c_void_p, _c.c_int, _c.c_float, _c.c_size_t, _c.c_double, _c.c_long


class ConvGeom(ctypes.Structure):
    """mi_conv_geom of include/cetpick_hip.h, fields in header order (tests/test_abi.py checks)"""
    _fields_ = [(f, _I) for f in "N Di Hi Wi Ci Co kd kh kw stride pd ph pw dd dh dw".split()]


_G = _c.POINTER(ConvGeom)


class Aug2d3dRanges(ctypes.Structure):
    """mi_aug2d3d_ranges of include/cetpick_hip.h, fields in header order"""
    _fields_ = [(f, _F) for f in "flip_p angle_lo angle_hi erase_p scale_lo scale_hi ratio_lo ratio_hi".split()]


_R = _c.POINTER(Aug2d3dRanges)


class Aug3dRanges(ctypes.Structure):
    """mi_aug3d_ranges of include/cetpick_hip.h, fields in header order"""
    _fields_ = [(f, _F) for f in ("blur_p sigma_lo sigma_hi noise_p noise_lo noise_hi rot_p angle_lo angle_hi flip_z_below "
                                  "flip_y_above drop_below centre_below swap_below").split()]


_R3 = _c.POINTER(Aug3dRanges)


class PlotLayout(ctypes.Structure):
    """mi_plot_layout of include/cetpick_hip.h, fields in header order"""
    _fields_ = [(f, _I) for f in "P M R T label_dx label_dy glyph_px glyph_gap box_pad box_border".split()]


_PL = _c.POINTER(PlotLayout)


class _S:
    """The `mi_stream_t stream` parameter in SIGNATURES: always the last one; bound as a void*, filled in by call()."""


# name -> (restype, argtypes); kept in step with include/cetpick_hip.h (tests/test_abi.py checks)
SIGNATURES = {
    "mi_abi_version": (_I, []),
    "mi_graph_node_counts": (_I, [_P, _P]),
    "mi_debug_stamp": (_I, [_P, _S]),
    "mi_linear_stats_fwd_f32": (_I, [_P] * 5 + [_I] * 3 + [_S]),
    "mi_debug_last_conv_kernel": (_c.c_char_p, []),
    "mi_debug_last_conv_plan": (_I, [_P, _I]),
    "mi_linear_bn_fwd_f32": (_I, [_P] * 5 + [_I] * 3 + [_P, _P, _F, _F] + [_P] * 4 + [_I, _S]),
    "mi_conv3d_stem_stats_workspace_bytes": (_Z, [_I] * 5),
    "mi_conv3d_stem_stats_f32": (_I, [_P, _P, _P] + [_I] * 5 + [_P, _P, _Z, _S]),
    "mi_build_arch": (_c.c_char_p, []),
    "mi_sigmoid_clamp": (_I, [_P, _P, _Z, _S]),
    "mi_nms3d": (_I, [_P, _P, _I, _I, _I, _I, _I, _S]),
    "mi_decode_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "mi_decode_workspace_init": (_I, [_P, _Z, _S]),
    "mi_sigmoid_nms_topk": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _S]),
    "mi_gauss3d_sep": (_I, [_P, _P, _P, _I, _I, _I, _F, _S]),
    "mi_dog_pick_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "mi_dog_pick": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _Z, _S]),
    "mi_greedy_nms3d_workspace_bytes": (_Z, [_I, _I, _I]),
    "mi_greedy_nms3d": (_I, [_P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _I, _P, _Z, _S]),
    "mi_crop_normalize": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _S]),
    "mi_crop_normalize_table": (_I, [_P, _P, _P, _P, _P, _c.c_int64, _I, _I, _I, _I, _I, _I, _P, _S]),
    "mi_u8_roundtrip_normalize": (_I, [_P, _P, _Z, _F, _F, _S]),
    # pose crops and pose pooling of the MoCo-3D exploration inference (csrc/crop_pose.hip)
    "mi_crop_znorm_poses": (_I, [_P, _P, _P, _c.c_int64, _I, _I, _I, _I, _P, _I, _P, _S]),
    "mi_embed_pool": (_I, [_P, _L, _I, _I, _P, _S]),
    "mi_aug2d_params": (_I, [_P, _c.c_int64, _c.c_uint64, _I, _I, _I] + [_F] * 7 + [_P, _S]),
    "mi_aug2d_apply": (_I, [_P, _c.c_int64, _I, _P, _P, _c.c_int64, _I, _F, _F, _P, _S]),
    "mi_aug2d3d_params": (_I, [_P, _c.c_int64, _c.c_uint64, _I, _I, _R, _R, _P, _S]),
    "mi_aug2d3d_apply": (_I, [_P, _P, _c.c_int64, _I, _P, _P, _P, _P, _c.c_int64, _I, _F, _F, _F, _F, _P, _S]),
    "mi_aug3d_params": (_I, [_P, _c.c_int64, _c.c_uint64, _I, _I, _I, _I, _R3, _P, _S]),
    "mi_aug3d_workspace_bytes": (_Z, [_c.c_int64, _I, _I]),
    "mi_aug3d_apply": (_I, [_P, _P, _P, _c.c_int64, _P, _P, _c.c_int64, _I, _I, _P, _P, _Z, _S]),
    "mi_tilt_patches": (_I, [_P, _I, _P, _P, _c.c_int64, _I, _I, _D, _D, _P, _P, _S]),
    "mi_semi_labels": (_I, [_P, _I, _I, _I, _P, _c.c_int64, _P, _I, _I, _S]),
    "mi_semi_pairs": (_I, [_P, _P, _I, _P, _P, _c.c_int64, _I, _I, _P, _P, _P, _S]),
    # training path
    "mi_gauss2d_slices": (_I, [_P, _P, _P, _I, _I, _I, _F, _S]),
    "mi_rec_reorder": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _S]),
    "mi_vol_stats_workspace_bytes": (_Z, [_L, _L]),
    "mi_vol_stats": (_I, [_P, _L, _L, _P, _P, _Z, _S]),
    "mi_zscore": (_I, [_P, _P, _L, _L, _P, _S]),
    "mi_zscore_quantize_minmax": (_I, [_P, _P, _L, _L, _P, _D, _D, _I, _S]),
    "mi_conv_workspace_bytes": (_Z, [_G]),
    "mi_conv_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _G, _P, _Z, _S]),
    "mi_conv_dgrad_f32": (_I, [_P, _P, _P, _P, _P, _G, _P, _Z, _S]),
    "mi_conv_wgrad_f32": (_I, [_P, _P, _P, _G, _P, _Z, _P, _S]),
    "mi_conv_wgrad_batch_f32": (_I, [_P, _P, _P, _P, _I, _G, _Z, _P, _S]),
    "mi_stem2d_fwd_bias_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _S]),
    "mi_upconv_tail_fwd": (_I, [_P, _P, _P, _P, _P] + [_I] * 7 + [_S]),
    "mi_smallk_image_bytes": (_Z, [_I, _I]),
    "mi_smallk_prep": (_I, [_P, _P, _I, _I, _S]),
    "mi_smallk_fwd_f32": (_I, [_P, _P, _P, _P, _I, _L, _I, _I, _I, _L, _I, _S]),
    "mi_smallk_heads_fwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _L, _I, _L, _I, _S]),
    "mi_splitk_reduce_batch": (_I, [_P, _P, _P, _P, _I, _S]),
    "mi_linear_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _S]),
    "mi_conv3d_direct_wimg_bytes": (_Z, [_I]),
    "mi_conv3d_direct_workspace_bytes": (_Z, [_I, _I]),
    "mi_conv3d_direct_usable": (_I, [_I] * 9),
    "mi_conv3d_direct_prep": (_I, [_P, _P, _P, _P, _I, _S]),
    "mi_conv3d_direct_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _Z, _S]),
    "mi_conv2d_p2d_usable": (_I, [_I] * 4),
    "mi_conv2d_p2d_wimg_bytes": (_Z, [_I]),
    "mi_conv2d_p2d_prep": (_I, [_P, _P, _P, _P, _I, _S]),
    "mi_conv2d_p2d_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _S]),
    "mi_conv2d_p2d_wgrad_workspace_bytes": (_Z, [_I] * 4),
    "mi_conv2d_p2d_wgrad_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _Z, _S]),
    "mi_conv2d_stem3_workspace_bytes": (_Z, [_I]),
    "mi_conv2d_stem3_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _S]),
    "mi_conv2d_stem3_wgrad_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _Z, _S]),
    "mi_conv3d_cube2_workspace_bytes": (_Z, [_I, _I]),
    "mi_conv3d_cube2_usable": (_I, [_I] * 9),
    "mi_conv3d_cube2_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _S]),
    "mi_conv_d32_kind": (_I, [_I] * 12),
    "mi_conv_d32_image_bytes": (_Z, [_I, _I]),
    "mi_conv_d64_image_bytes": (_Z, [_I, _I]),
    "mi_conv_d32_prep": (_I, [_P, _P, _I, _I, _S]),
    "mi_conv_d64_prep_co": (_I, [_P, _P, _I, _I, _I, _S]),
    "mi_conv_d32_1x1_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _S]),
    "mi_conv_d32_fwd_pool_f32": (_I, [_P, _P, _P, _P, _P] + [_I] * 7 + [_S]),
    "mi_conv_d32_fwd_pool_strided_f32": (_I, [_P, _P, _P, _P, _I, _P] + [_I] * 7 + [_S]),
    "mi_copy_channels_into": (_I, [_P, _I, _P, _I, _I, _L, _S]),
    "mi_conv_d32_upconv_fwd_f32": (_I, [_P, _P, _P, _P, _P] + [_I] * 8 + [_S]),
    "mi_conv_d64_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _S]),
    "mi_conv_d32_fwd_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _S]),
    "mi_maxpool2d_ceil_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _S]),
    "mi_maxpool2d_ceil_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _S]),
    "mi_shuffle2x2_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _S]),
    "mi_shuffle2x2_bwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _S]),
    "mi_concat_channels": (_I, [_P, _I, _P, _I, _P, _L, _S]),
    "mi_split_channels": (_I, [_P, _P, _I, _P, _I, _L, _S]),
    "mi_zhead_fwd": (_I, [_P, _P, _P, _I, _I, _L, _I, _I, _S]),
    "mi_zhead_bwd_workspace_bytes": (_Z, [_I, _I, _L, _I, _I]),
    "mi_zhead_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _L, _I, _I, _P, _Z, _S]),
    "mi_voxel_loss_workspace_bytes": (_Z, [_L]),
    "mi_pu_focal_loss_fwd": (_I, [_P, _P, _L, _D, _D, _P, _P, _P, _Z, _S]),
    "mi_pu_focal_loss_bwd": (_I, [_P, _P, _L, _D, _P, _P, _P, _S]),
    "mi_focal_loss_fwd": (_I, [_P, _P, _L, _P, _P, _P, _Z, _S]),
    "mi_focal_loss_bwd": (_I, [_P, _P, _L, _P, _P, _P, _S]),
    "mi_pu_ge_loss_workspace_bytes": (_Z, [_L]),
    "mi_pu_ge_loss_fwd": (_I, [_P, _P, _L, _D, _D, _D, _P, _P, _P, _Z, _S]),
    "mi_pu_ge_loss_bwd": (_I, [_P, _P, _L, _D, _P, _P, _P, _S]),
    "mi_mse_loss_fwd": (_I, [_P, _P, _L, _P, _P, _P, _Z, _S]),
    "mi_mse_loss_bwd": (_I, [_P, _P, _L, _P, _P, _P, _P, _S]),
    "mi_ucl_rowsums_fwd": (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _S]),
    "mi_ucl_rowsums_bwd_ranged": (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _S]),
    "mi_supcon_pn_rows_workspace_bytes": (_Z, [_I]),
    "mi_supcon_pn_rows_fwd": (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _Z, _S]),
    "mi_supcon_pn_rows_bwd": (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _S]),
    "mi_colreduce_workspace_bytes": (_Z, [_L, _I]),
    "mi_bn_stats": (_I, [_P, _L, _I, _P, _P, _Z, _S]),
    "mi_bn_apply_fwd": (_I, [_P, _P, _L, _I, _P, _D, _P, _P, _F, _F, _P, _P, _P, _P, _P, _I, _S]),
    "mi_bn_relu_maxpool3d_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _D, _P, _P, _F, _F, _P, _P, _P, _P, _S]),
    "mi_bn_relu_bwd_reduce_x": (_I, [_P, _P, _L, _I, _P, _P, _P, _P, _P, _Z, _S]),
    "mi_bn_relu_bwd_apply_x": (_I, [_P, _P, _P, _L, _I, _P, _P, _P, _P, _D, _P, _P, _S]),
    "mi_bn_small_fwd": (_I, [_P, _P, _L, _I, _P, _P, _F, _F, _P, _P, _P, _P, _P, _I, _S]),
    "mi_bn_small_bwd": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, _I, _P, _P, _S]),
    "mi_bn_small_pool_fwd": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _F, _F, _P, _P, _P, _P, _S]),
    "mi_bn_small_pool_bwd": (_I, [_P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P, _S]),
    "mi_bn_eval_fwd": (_I, [_P, _P, _L, _I, _P, _P, _P, _P, _F, _P, _P, _I, _S]),
    "mi_bn_bwd_reduce": (_I, [_P, _P, _P, _L, _I, _P, _I, _P, _P, _Z, _S]),
    "mi_bn_bwd_apply": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, _P, _D, _I, _P, _P, _S]),
    "mi_bn_bwd_apply_res": (_I, [_P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _D, _P, _P, _S]),
    "mi_bn_param_grads": (_I, [_P, _I, _P, _P, _S]),
    "mi_colsum": (_I, [_P, _L, _I, _P, _P, _P, _Z, _S]),
    "mi_maxpool3d_fwd": (_I, [_P, _P, _P] + [_I] * 8 + [_S]),
    "mi_maxpool3d_bwd": (_I, [_P, _P, _P] + [_I] * 8 + [_S]),
    "mi_avgpool_fwd": (_I, [_P, _P, _I, _I, _I, _S]),
    "mi_avgpool_bwd": (_I, [_P, _P, _I, _I, _I, _S]),
    "mi_bias_add": (_I, [_P, _P, _L, _I, _S]),
    "mi_copy_pair_f32": (_I, [_P, _P, _P, _P, _L, _S]),
    "mi_relu_mask": (_I, [_P, _P, _P, _P, _L, _S]),
    "mi_l2norm_fwd": (_I, [_P, _P, _P, _I, _I, _S]),
    "mi_l2norm_bwd": (_I, [_P, _P, _P, _P, _I, _I, _S]),
    "mi_moco_logits_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _S]),
    "mi_moco_logits_norm_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _S]),
    "mi_moco_logits_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _S]),
    "mi_rowdot_mean_fwd": (_I, [_P, _P, _P, _I, _I, _S]),
    "mi_rowdot_mean_bwd": (_I, [_P, _P, _P, _I, _I, _S]),
    "mi_column_std_mean": (_I, [_P, _P, _I, _I, _S]),
    "mi_ce_label0_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _S]),
    "mi_ce_label0_bwd": (_I, [_P, _P, _P, _P, _I, _I, _S]),
    "mi_conv3d_s2_dgrad_usable": (_I, [_I, _I, _I, _I]),
    "mi_conv3d_s2_dgrad_workspace_bytes": (_Z, [_I, _I]),
    "mi_conv3d_s2_dgrad_f32": (_I, [_P] * 7 + [_I, _I, _I, _I, _P, _Z, _S]),
    "mi_conv3d_s2_fwd_usable": (_I, [_I, _I, _I, _I]),
    "mi_conv3d_s2_fwd_workspace_bytes": (_Z, [_I, _I]),
    "mi_conv3d_s2_fwd_f32": (_I, [_P] * 5 + [_I, _I, _I, _I, _P, _Z, _S]),
    "mi_conv3d_s2_prep": (_I, [_P] * 6 + [_I, _S]),
    "mi_conv3d_s2_fwd_img_f32": (_I, [_P] * 4 + [_I] * 4 + [_S]),
    "mi_conv3d_s2_dgrad_img_f32": (_I, [_P] * 6 + [_I] * 4 + [_S]),
    "mi_ema_update": (_I, [_P, _P, _F, _L, _S]),
    "mi_sgd_step": (_I, [_P, _P, _P, _F, _F, _F, _L, _S]),
    "mi_sgd_step2": (_I, [_P, _P, _P, _P, _F, _F, _F, _L, _S]),
    "mi_scalar_accumulate": (_I, [_P, _P, _P, _P, _P, _S]),
    "mi_queue_enqueue": (_I, [_P, _P, _P, _I, _I, _I, _S]),
    # k-means over the exploration embeddings (csrc/kmeans.hip)
    "mi_kmeans_image_bytes": (_Z, [_I, _I]),
    "mi_kmeans_workspace_bytes": (_Z, [_L, _I, _I]),
    "mi_kmeans_prep": (_I, [_P, _I, _I, _P, _S]),
    "mi_kmeans_xnorm": (_I, [_P, _L, _I, _P, _S]),
    "mi_kmeans_assign": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _P, _Z, _S]),
    "mi_kmeans_update": (_I, [_P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _Z, _S]),
    # k-nearest-neighbour search over embeddings (csrc/knn.hip)
    "mi_knn_image_bytes": (_Z, [_L, _I]),
    "mi_knn_workspace_bytes": (_Z, [_L, _L, _I, _I, _I, _I]),
    "mi_knn_search": (_I, [_P, _P, _L, _L, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _S]),
    # t-SNE over the neighbour graph (csrc/tsne.hip)
    "mi_tsne_affinities": (_I, [_P, _L, _I, _F, _P, _P, _S]),
    "mi_tsne_workspace_bytes": (_Z, [_L, _I, _I]),
    "mi_tsne_gradient": (_I, [_P, _P, _P, _P, _P, _L, _I, _F, _I, _P, _P, _P, _P, _Z, _S]),
    "mi_tsne_update": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _S]),
    # UMAP over the neighbour graph (csrc/umap.hip)
    "mi_umap_check": (_I, [_L, _I]),
    "mi_umap_smooth_knn": (_I, [_P, _L, _I, _D, _P, _P, _P, _S]),
    "mi_umap_union": (_I, [_P, _P, _P, _P, _L, _I, _P, _I, _P, _P, _P, _S]),
    "mi_umap_rowmax": (_I, [_P, _P, _P, _P, _P, _L, _I, _D, _D, _P, _S]),
    "mi_umap_supervise": (_I, [_P, _P, _P, _P, _L, _I, _D, _D, _P, _I, _P, _P, _S]),
    "mi_umap_epoch": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _D, _D, _c.c_uint64, _S]),
    # the spectral start of the UMAP map (csrc/spectral.hip)
    "mi_graph_components": (_I, [_P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _S]),
    "mi_spectral_degree": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _P, _P, _S]),
    "mi_spectral_spmv": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _L, _L, _S]),
    "mi_spectral_workspace_bytes": (_Z, [_I, _L]),
    "mi_spectral_dots": (_I, [_P, _L, _I, _L, _P, _P, _P, _Z, _S]),
    "mi_spectral_orth": (_I, [_P, _L, _I, _L, _P, _P, _P, _Z, _S]),
    "mi_spectral_combine": (_I, [_P, _L, _I, _L, _P, _P, _D, _S]),
    # colours of the map, 8-bit Gaussian and disc painter of the 3-D visualisation (csrc/vis3d.hip)
    "mi_vis_sample_colours": (_I, [_P, _L, _P, _I, _I, _P, _S]),
    "mi_vis_slice_bytes": (_I, [_P, _L, _L, _P, _D, _D, _P, _S]),
    "mi_vis_gauss_workspace_bytes": (_Z, [_L, _L, _L]),
    "mi_vis_gauss_u8": (_I, [_P, _I, _I, _I, _P, _P, _P, _Z, _S]),
    "mi_vis_paint": (_I, [_P, _P, _L, _P, _I, _I, _I, _I, _I, _I, _P, _P, _S]),
    # thumbnail selection, thumbnails, grey patch bytes and the map pictures (csrc/plot2d.hip)
    "mi_plot_select_workspace_bytes": (_Z, [_L, _F]),
    "mi_plot_select": (_I, [_P, _L, _F, _P, _P, _P, _Z, _S]),
    "mi_plot_thumbs": (_I, [_P, _L, _I, _I, _P, _L, _I, _P, _P, _S]),
    "mi_plot_patch_bytes": (_I, [_P, _L, _I, _I, _P, _P, _S]),
    "mi_plot_raster_workspace_bytes": (_Z, [_I]),
    "mi_plot_raster": (_I, [_P, _L, _P, _L, _P, _P, _P, _P, _PL, _I, _P, _P, _Z, _S]),
    # slice pictures of the detector's validation, --debug 4 (csrc/debug_vis.hip)
    "mi_dbgvis_minmax": (_I, [_P, _I, _I, _I, _I, _I, _P, _S]),
    "mi_dbgvis_workspace_bytes": (_Z, [_I, _L, _L]),
    "mi_dbgvis_render": (_I, [_P, _P, _P] + [_I] * 7 + [_P, _P, _L, _P, _L, _F, _I, _P, _P, _Z, _S]),
    # optimal matching of picks to target centres (csrc/match.hip)
    "mi_match_workspace_bytes": (_Z, [_I, _I, _I]),
    "mi_match_coordinates": (_I, [_P, _P, _P, _P, _I, _D, _P, _P, _P, _P, _Z, _S]),
    # distance-graph components of the picks and the per-component quadratic fits, --spike / --fiber (csrc/pick_groups.hip)
    "mi_pick_workspace_bytes": (_Z, [_I]),
    "mi_pick_components": (_I, [_P, _I, _D, _P, _P, _P, _Z, _S]),
    "mi_pick_fiber_fit": (_I, [_P, _I, _P, _P, _D, _D, _D, _P, _P, _I, _P, _P, _Z, _S]),
    # per-class mean, deviation, count and exemplars of the picks' patches, and their picture (csrc/class_gallery.hip)
    "mi_gallery_workspace_bytes": (_Z, [_L, _I, _I, _I]),
    "mi_gallery_moments": (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _Z, _S]),
    "mi_gallery_exemplars": (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _Z, _S]),
    "mi_gallery_raster_workspace_bytes": (_Z, [_I, _I]),
    "mi_gallery_raster": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _I, _P, _Z, _S]),
    # the SCAN loss over all heads, its gradient, and the class assignment (csrc/scan_loss.hip)
    "mi_scan_loss_workspace_bytes": (_Z, [_I, _I, _I]),
    "mi_scan_loss_fwd": (_I, [_P, _P, _I, _I, _I, _D, _P, _P, _P, _P, _Z, _S]),
    "mi_scan_loss_bwd": (_I, [_P, _P, _I, _I, _I, _D, _P, _P, _P, _P, _S]),
    "mi_scan_assign": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _S]),
    # the heads scored over the whole graph and the self-labelling loss (csrc/scan_selflabel.hip)
    "mi_scan_graph_eval_workspace_bytes": (_Z, [_L, _I, _I]),
    "mi_scan_graph_eval": (_I, [_P, _L, _I, _I, _P, _I, _I, _P, _P, _P, _Z, _S]),
    "mi_scan_selflabel_workspace_bytes": (_Z, [_I, _I]),
    "mi_scan_selflabel_fwd": (_I, [_P, _P, _I, _I, _D, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _S]),
    "mi_scan_selflabel_bwd": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _S]),
    # the exact silhouette of a clustering and the contingency table of two (csrc/cluster_quality.hip)
    "mi_silhouette_workspace_bytes": (_Z, [_L, _I, _I]),
    "mi_silhouette_sums": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _Z, _S]),
    "mi_silhouette_finalise_workspace_bytes": (_Z, [_L, _I, _I]),
    "mi_silhouette_finalise": (_I, [_P, _P, _P, _L, _I, _I] + [_P] * 10 + [_Z, _S]),
    "mi_label_contingency": (_I, [_P, _P, _L, _I, _I, _P, _S]),
    # label spreading over the neighbour graph and the seed matching (csrc/label_spread.hip)
    "mi_spread_weights": (_I, [_P, _P, _L, _I, _I, _P, _P, _S]),
    "mi_spread_csr_count": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, _S]),
    "mi_spread_csr_fill": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, _L, _P, _P, _S]),
    "mi_spread_step": (_I, [_P, _P, _P, _L, _I, _D, _P, _P, _P, _P, _S]),
    "mi_spread_decide": (_I, [_P, _L, _I, _D, _P, _P, _P, _S]),
    "mi_seed_nearest": (_I, [_P, _P, _L, _P, _P, _L, _D, _P, _P, _S]),
}

_lib = None


class HipExtensionError(RuntimeError):
    pass


def lib():
    """The loaded shared library (loads on first use; raises if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionError(
                "%s is missing: run `python -m cet_pick_amd.build` (there is no CPU fallback)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = [_P if a is _S else a for a in args]
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        kind = {-1: "bad argument", -2: "workspace too small", -3: "unsupported"}.get(rc, "hipError %d" % rc)
        raise HipExtensionError("%s failed: %s" % (what, kind))


# name -> (takes a stream, positions of its void* parameters: the only places where a tensor may stand)
_ENTRIES = {name: (bool(args) and args[-1] is _S, tuple(i for i, a in enumerate(args) if a is _P))
            for name, (_, args) in SIGNATURES.items()}
_Tensor = torch.Tensor


def call(name, *args, may_decline=False):
    """Launch the entry `name`: the one way product code starts a kernel.  A tensor, where the header has a void* or a typed data
    pointer, goes in as its device address (one on the host raises: its address inside a kernel is a GPU fault), None as NULL,
    everything else as it is (a tensor anywhere else is refused by ctypes); an entry that takes a stream gets the current one
    appended; a non-zero status raises.  Returns True - or False, with `may_decline`, when the entry answers -3 (MI_E_UNSUPPORTED)
    and the caller has another route.  (Only the pointer positions are looked at: the scalars of a launch cost nothing here.)"""
    try:
        streamed, pointers = _ENTRIES[name]
    except KeyError:
        raise HipExtensionError("%s is not an entry of include/cetpick_hip.h" % name) from None
    argv = [*args, stream()] if streamed else list(args)
    try:
        for i in pointers:
            a = argv[i]
            if isinstance(a, _Tensor):
                if not a.is_cuda:
                    raise HipExtensionError("%s: argument %d is a tensor on %s, not on the MI355X (cuda) device; there is no CPU path"
                                            % (name, i, a.device))
                argv[i] = a.data_ptr()      # a plain integer: argtypes makes the void* of it
    except IndexError:
        raise HipExtensionError("%s takes %d arguments, got %d" % (name, len(SIGNATURES[name][1]) - streamed, len(args))) from None
    rc = getattr(_lib if _lib is not None else lib(), name)(*argv)
    if rc:
        if rc == -3 and may_decline:
            return False
        check(rc, name)
    return True


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def host_array(vals, ctype=ctypes.c_void_p):
    """A host array of device pointers / ints as the void* the C-ABI's array arguments take (the cast keeps the array alive)."""
    return ctypes.cast((ctype * len(vals))(*vals), ctypes.c_void_p)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(t, name="tensor", dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipExtensionError("%s must be a tensor on the MI355X (cuda) device; there is no CPU path" % name)
    if dtype is not None and t.dtype != dtype:
        raise HipExtensionError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t


_workspaces = {}


def _ws_key(device, tag):
    return (str(device), tag, torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0)


def workspace(nbytes, device, tag="default", init=None):
    """A cached device scratch buffer of at least nbytes (grown geometrically, never shrunk).
    `init(buf)` runs once per (re)allocation - for workspaces whose header is kept clean from call to call."""
    # one buffer per (device, purpose, stream): launches on different streams must not share scratch
    key = _ws_key(device, tag)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        if init is not None:
            init(buf)
            _ws_inits[key] = init
        _workspaces[key] = buf
    return buf


_ws_inits = {}


def prime_workspaces_for_stream(src_stream, dst_stream):
    """Give `dst_stream` its own copy of every kept-clean (init) workspace `src_stream` has, initialised NOW: a step engine calls this
    in front of a hipGraph capture on `dst_stream` - workspaces are keyed by stream, and one that is first allocated inside the capture
    has its initialising fill recorded as a node that replays with every step (2.6 MB of zeros for cube2_kernel's arrival counters)."""
    src, dst = src_stream.cuda_stream, dst_stream.cuda_stream
    if src == dst:
        return
    with torch.cuda.stream(dst_stream):
        for key in [k for k in _workspaces if k[2] == src and k in _ws_inits]:
            nk = (key[0], key[1], dst)
            if nk in _workspaces and _workspaces[nk].numel() >= _workspaces[key].numel():
                continue
            buf = torch.empty(_workspaces[key].numel(), dtype=torch.uint8, device=_workspaces[key].device)
            _ws_inits[key](buf)
            _workspaces[nk], _ws_inits[nk] = buf, _ws_inits[key]
    dst_stream.synchronize()


def drop_workspace(device, tag):
    """Forget a cached workspace (after a failed call its kept-clean header can no longer be trusted)."""
    _workspaces.pop(_ws_key(device, tag), None)
    _ws_inits.pop(_ws_key(device, tag), None)
