"""ctypes binding of libvatl_hip.so (include/vatl_hip.h) + thin torch-tensor wrappers.

PyTorch is plumbing only: it owns device memory and the HIP stream; every
wrapper passes ``tensor.data_ptr()`` and the current stream to the C ABI.
There is NO fallback: a missing library or a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading as _threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# VATL_HIP_LIB: an explicit library path — the profiling variant (build.py --ablation) for tools/conv_bench.py --ablate
LIB_PATH = os.environ.get("VATL_HIP_LIB") or os.path.join(_HERE, "libvatl_hip.so")

_p = C.c_void_p
_i = C.c_int
_f = C.c_float
_d = C.c_double
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/vatl_hip.h one to one
# (tests/test_cabi.py parses the header and checks this table against it)
SIGNATURES = {
    "vatl_version": (_i, []),
    "vatl_last_error": (C.c_char_p, []),
    "vatl_flop_meter_begin": (_i, []),
    "vatl_flop_meter_end": (_i, [_p, _p, _p, _p]),
    "vatl_flop_meter_routes": (_i, [_p, _i]),
    "vatl_nchw_to_nhwc": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_nhwc_to_nchw": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_pack_conv_weight": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_pack_deconv4x4s2_weight": (_i, [_p, _p, _i, _i, _i, _p]),
    "vatl_pack_conv1x1_dual_weight": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_conv1x1_dual_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_winograd_c32_weight_floats": (_i64, []),
    "vatl_pack_winograd_c32_weight": (_i, [_p, _p, _p]),
    "vatl_conv3x3_winograd_c32_supported": (_i, [_i, _i, _i, _i, _i]),
    "vatl_conv3x3_winograd_c32_fwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_winograd_f4_weight_floats": (_i64, [_i, _i]),
    "vatl_pack_winograd_f4_weight": (_i, [_p, _p, _i, _i, _i, _p]),
    "vatl_winograd_f4_stats_row_blocks": (_i64, [_i64, _i, _i]),
    "vatl_conv3x3_winograd_f4_fwd_stats": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_conv3x3_winograd_f4_fwd_bnbwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "vatl_conv3x3_winograd_f4_supported": (_i, [_i, _i, _i, _i, _i]),
    "vatl_conv3x3_winograd_f4_fwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_conv1x1_rows_supported": (_i, [_i, _i, _i, _i64]),
    "vatl_conv1x1_rows_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _p]),
    "vatl_bottleneck_chain_supported": (_i, [_i, _i, _i, _i64]),
    "vatl_bottleneck_chain_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "vatl_chain_proj_supported": (_i, [_i, _i, _i, _i64]),
    "vatl_chain_proj_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _p]),
    "vatl_chain_step_supported": (_i, [_i, _i, _i, _i64]),
    "vatl_chain_step_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "vatl_stem_pool_weight_floats": (_i64, []),
    "vatl_pack_stem_pool_weight": (_i, [_p, _p, _p]),
    "vatl_stem_pool_supported": (_i, [_i, _i]),
    "vatl_stem_pool_w1d_weight_floats": (_i64, []),
    "vatl_pack_stem_pool_w1d_weight": (_i, [_p, _p, _p]),
    "vatl_stem_pool_w1d_supported": (_i, [_i, _i]),
    "vatl_stem7x7s2_pool_w1d_fwd": (_i, [_p] * 5 + [_i] * 3 + [_p]),
    "vatl_stem7x7s2_pool_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "vatl_stem3_weight_floats": (_i64, []),
    "vatl_pack_stem3_weight": (_i, [_p, _p, _p]),
    "vatl_stem3x3s2_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "vatl_bn_fold": (_i, [_p, _p, _p, _p, _p, _f, _p, _p, _i, _p]),
    "vatl_tune_set": (_i, [_i, _i]),
    "vatl_set_splitk_workspace": (_i, [_p, _i64]),
    "vatl_set_splitk_workspace_thread": (_i, [_p, _i64]),
    "vatl_streamk_workspace_bytes": (_i64, []),
    "vatl_set_streamk_workspace_thread": (_i, [_p, _i64]),
    "vatl_conv_cout_pad": (_i, [_i]),
    "vatl_conv2d_fwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_deconv4x4s2_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_maxpool3x3s2_fwd": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_gap_fwd": (_i, [_p, _p, _i, _i, _i, _p]),
    "vatl_pixelshuffle2_fwd": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_se_scale_add_relu": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "vatl_fuse_upsample_add": (_i, [_p, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_upsample_nearest_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_gap_bwd": (_i, [_p, _p, _i, _i, _i, _p]),
    "vatl_flip_nchw": (_i, [_p, _p, C.c_int64, _i, _p]),
    "vatl_flip_merge": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_decode_argmax_affine": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_decode_pose": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_thc_pairs": (_i, [_p, _p, _i64, _i64, _p, _i, _i, _i, _i, _p]),
    "vatl_thc_combine": (_i, [_p, _p, _p, _p, _i, _p]),
    "vatl_localpeak_mean": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _f, _p]),
    "vatl_hybrid_ae_wpu": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _i, _p]),
    "vatl_tpc_stream": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "vatl_decode_softargmax": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_ae_forward": (_i, [_p, _p, _i, _i, _p, _p, _i, _p]),
    "vatl_hybrid_feature_f64": (_i, [_p, _p, _p, _p, _i, _p]),
    "vatl_localpeak_mask": (_i, [_p, _p, _i, _i, _i, _f, _p]),
    "vatl_peaks5": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_plane_entropy": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_conv2d_fwd_ex": (_i, [_p] * 6 + [_i] * 20 + [_p]),
    "vatl_conv2d_fwd_ex_bnbwd": (_i, [_p] * 4 + [_i] * 19 + [_p] * 9),
    "vatl_bn_bwd_from_stats": (_i, [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _p, _p]),
    "vatl_pack_dgrad_weight": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "vatl_conv2d_wgrad_workspace_floats": (_i64, [_i, _i, _i, _i, _i64]),
    "vatl_conv2d_wgrad": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_deconv4x4s2_wgrad_workspace_floats": (_i64, [_i, _i, _i64]),
    "vatl_deconv4x4s2_wgrad": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_col_reduce_workspace_doubles": (_i64, [_i64, _i]),
    "vatl_bn_train_fwd_stats": (_i, [_p, _i64, _i, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _p]),
    "vatl_scale_bias_act": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _p]),
    "vatl_bn_train_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _p, _p, _p]),
    "vatl_bn_train_bwd_relu": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _p, _p, _p]),
    "vatl_conv_stats_row_blocks": (_i64, [_i64, _i]),
    "vatl_winograd_cout_pad": (_i, [_i]),
    "vatl_winograd_weight_floats": (_i64, [_i, _i]),
    "vatl_pack_winograd_weight": (_i, [_p, _p, _i, _i, _i, _p]),
    "vatl_conv3x3_winograd_fwd": (_i, [_p] * 6 + [_i] * 6 + [_p]),
    "vatl_winograd_last_route": (_i, []),
    "vatl_winograd_stats_row_blocks": (_i64, [_i64, _i, _i]),
    "vatl_conv3x3_winograd_fwd_stats": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_conv3x3_winograd_fwd_bnbwd": (_i, [_p] * 4 + [_i] * 5 + [_p] * 9),
    "vatl_conv3x3_winograd_wgrad_workspace_floats": (_i64, [_i, _i, _i64, _i, _i]),
    "vatl_conv3x3_winograd_wgrad": (_i, [_p] * 4 + [_i] * 5 + [_p]),
    "vatl_deconv4x4s2_winograd_wgrad_workspace_floats": (_i64, [_i, _i, _i64, _i, _i]),
    "vatl_deconv4x4s2_winograd_wgrad": (_i, [_p] * 4 + [_i] * 5 + [_p]),
    "vatl_winograd_deconv_dgrad_weight_floats": (_i64, [_i, _i]),
    "vatl_pack_winograd_deconv_dgrad_weight": (_i, [_p, _p, _i, _i, _p]),
    "vatl_deconv4x4s2_winograd_dgrad": (_i, [_p] * 4 + [_i] * 5 + [_p]),
    "vatl_deconv4x4s2_winograd_dgrad_bnbwd": (_i, [_p] * 4 + [_i] * 5 + [_p] * 9),
    "vatl_winograd_deconv_weight_floats": (_i64, [_i, _i]),
    "vatl_pack_winograd_deconv_weight": (_i, [_p, _p, _i, _i, _p]),
    "vatl_deconv4x4s2_winograd_fwd": (_i, [_p] * 5 + [_i] * 6 + [_p]),
    "vatl_winograd_deconv43_weight_floats": (_i64, [_i, _i]),
    "vatl_pack_winograd_deconv43_weight": (_i, [_p, _p, _i, _i, _p]),
    "vatl_deconv4x4s2_winograd43_supported": (_i, [_i, _i, _i, _i, _i]),
    "vatl_deconv4x4s2_winograd43_fwd": (_i, [_p] * 5 + [_i] * 6 + [_p]),
    "vatl_winograd_s2_43_weight_floats": (_i64, [_i, _i]),
    "vatl_pack_winograd_s2_43_weight": (_i, [_p, _p, _i, _i, _p]),
    "vatl_conv3x3s2_winograd43_supported": (_i, [_i, _i, _i, _i, _i]),
    "vatl_conv3x3s2_winograd43_fwd": (_i, [_p] * 5 + [_i] * 6 + [_p]),
    "vatl_gemm1x1_bf16x6_weight_floats": (_i64, [_i, _i]),
    "vatl_pack_gemm1x1_bf16x6_weight": (_i, [_p, _p, _i, _i, _p]),
    "vatl_gemm1x1_bf16x6_supported": (_i, [_i64, _i, _i, _i]),
    "vatl_gemm1x1_bf16x6_fwd": (_i, [_p] * 6 + [_i] * 7 + [_p]),
    "vatl_gemm1x1_bf16x6_dual_fwd": (_i, [_p] * 6 + [_i] * 10 + [_p]),
    "vatl_gemm1x1_bf16x6_short_supported": (_i, [_i64, _i, _i]),
    "vatl_gemm1x1_bf16x6_short_fwd": (_i, [_p] * 6 + [_i] * 7 + [_p]),
    "vatl_winograd_deconv_stats_row_blocks": (_i64, [_i64, _i, _i]),
    "vatl_deconv4x4s2_winograd_fwd_stats": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_conv2d_fwd_stats": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_deconv4x4s2_fwd_stats": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_bn_train_finalize": (_i, [_p, _i64, _i64, _i, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p]),
    "vatl_maxpool3x3s2_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_maxpool3x3s2_fwd_idx": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_pack_weights_multi": (_i, [_p, _i, _i64, _p]),
    "vatl_adamw_multi_block_elems": (_i64, []),
    "vatl_checksum_block_words": (_i64, []),
    "vatl_checksum_multi": (_i, [_p, _i, _i64, _p, _p]),
    "vatl_maxpool3x3s2_fwd_idx_affine": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_bn_train_bwd_relu_pool": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "vatl_maxpool3x3s2_bwd_idx": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_pixelunshuffle2": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_se_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "vatl_relu_bwd": (_i, [_p, _p, _p, _i64, _p]),
    "vatl_col_sum": (_i, [_p, _i64, _i, _p, _p, _p]),
    "vatl_deform_conv2d_supported": (_i, [_i, _i, _i, _i]),
    "vatl_deform_conv2d_fwd": (_i, [_p, _p, _p, _i, _p, _i, _i, _p, _p, _p] + [_i] * 8 + [_p]),
    "vatl_deform_columns": (_i, [_p, _p, _i, _p, _i, _i, _p, _i] + [_i] * 6 + [_p]),
    "vatl_deform_columns_bwd": (_i, [_p, _i, _p, _p, _i, _p, _i, _i, _p, _p, _i, _p, _i] + [_i] * 6 + [_p]),
    "vatl_deform_dx_index_bytes": (_i64, [_i] * 5),
    "vatl_deform_columns_bwd_ordered": (_i, [_p, _i, _p, _p, _i, _p, _i, _i, _p, _p, _i, _p, _i] + [_i] * 6 + [_p, _i64, _p]),
    "vatl_masked_mse_workspace_floats": (_i64, [_i64]),
    "vatl_masked_mse_fwd_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "vatl_l1_joint_regression_fwd_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_gaussian_targets": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p]),
    "vatl_crop_warp_affine": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _f, _p]),
    "vatl_jpeg_probe": (_i, [_p, _i64, _p]),
    "vatl_jpeg_entropy_decode": (_i, [_p, _i64, _p, _i64, _p, _p]),
    "vatl_jpeg_pixels": (_i, [_p, _p, _p, _i, _i64, _i64, _p, _p, _i64, _p]),
    "vatl_jpeg_pack_size": (_i, [_p, _i64, _p, _p]),
    "vatl_jpeg_pack": (_i, [_p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _p]),
    "vatl_jpeg_huffman_workspace_bytes": (_i64, [_i64, _i64]),
    "vatl_jpeg_huffman": (_i, [_p, _p, _p, _p, _i, _i64, _i64, _i, _p, _i64, _p, _p, _i64, _p]),
    "vatl_ae_train_step": (_i, [_p, _p, _p, _p, _i, _i, _i, _d, _d, _d, _d, _i, _p, _p]),
    "vatl_ae_grad_workspace_floats": (_i64, [_i, _i, _i]),
    "vatl_ae_backward": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "vatl_ae_train_step_large": (_i, [_p, _p, _p, _p, _i, _i, _i, _d, _d, _d, _d, _d, _i, _i, _p, _p, _p]),
    "vatl_adamw_step": (_i, [_p, _p, _p, _p, _i64, _d, _d, _d, _d, _d, _i, _p]),
    "vatl_oks": (_i, [_p, _p, _p, _p, _i, _p]),
    "vatl_cosine_rowsum": (_i, [_p, _i64, _i, _p, _p, _p]),
    "vatl_kcenter_update": (_i, [_p, _i64, _i, _p, _i, _p, _i, _p]),
    "vatl_kcenter_pick": (_i, [_p, _p, _d, _d, _p, _i, _i64, _p]),
    "vatl_kmeans_prepare": (_i, [_p, _i64, _i, _p, _p, _p, _p, _p]),
    "vatl_kmeans_seed_workspace_doubles": (_i64, [_i64, _i]),
    "vatl_kmeans_seed": (_i, [_p, _p, _i64, _i, _i, _i, _p, _i, _p, _p, _p, _p]),
    "vatl_kmeans_assign": (_i, [_p, _p, _i64, _i, _i, _p, _p, _p, _p, _p]),
    "vatl_kmeans_update_workspace_doubles": (_i64, [_i, _i]),
    "vatl_kmeans_update": (_i, [_p, _p, _p, _p, _i64, _i, _i, _p, _p, _p, _p]),
    "vatl_kmeans_finish": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _i, _p, _p, _p, _p]),
    "vatl_adamw_step_multi": (_i, [_p, _i, _i64, _d, _d, _d, _d, _d, _i, _p]),
    "vatl_adam_step": (_i, [_p, _p, _p, _p, _i64, _d, _d, _d, _d, _d, _i, _p]),
    "vatl_adam_step_multi": (_i, [_p, _i, _i64, _d, _d, _d, _d, _d, _i, _p]),
    "vatl_rmsprop_step": (_i, [_p, _p, _p, _i64, _d, _d, _d, _d, _p]),
    "vatl_rmsprop_step_multi": (_i, [_p, _i, _i64, _d, _d, _d, _d, _p]),
    "vatl_sgd_step": (_i, [_p, _p, _p, _i64, _d, _d, _d, _i, _p]),
    "vatl_sgd_step_multi": (_i, [_p, _i, _i64, _d, _d, _d, _i, _p]),
    "vatl_pack_conv_weight_f64": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_pack_deconv4x4s2_weight_f64": (_i, [_p, _p, _i, _i, _p]),
    "vatl_conv2d_fwd_f64": (_i, [_p] * 6 + [_i] * 11 + [_p]),
    "vatl_deconv4x4s2_fwd_f64": (_i, [_p] * 5 + [_i] * 6 + [_p]),
    "vatl_nchw_to_nhwc_f64": (_i, [_p, _i, _p, _i, _i, _i, _i, _p]),
    "vatl_nhwc_to_nchw_f64": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_maxpool3x3s2_fwd_f64": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_gap_fwd_f64": (_i, [_p, _p, _i, _i, _i, _p]),
    "vatl_pixelshuffle2_fwd_f64": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_se_scale_add_relu_f64": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "vatl_fuse_upsample_add_f64": (_i, [_p, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_pack_conv_weight_h16": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_pack_deconv4x4s2_weight_h16": (_i, [_p, _p, _i, _i, _i, _p]),
    "vatl_conv2d_fwd_h16": (_i, [_p] * 6 + [_i] * 12 + [_p]),
    "vatl_deconv4x4s2_fwd_h16": (_i, [_p] * 5 + [_i] * 7 + [_p]),
    "vatl_nchw_to_nhwc_h16": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_nhwc_to_nchw_h16": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_maxpool3x3s2_fwd_h16": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_gap_fwd_h16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "vatl_pixelshuffle2_fwd_h16": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_se_scale_add_relu_h16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_fuse_upsample_add_h16": (_i, [_p, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
    "vatl_wgrad_h16_splits": (_i64, [_i64]),
    "vatl_conv2d_wgrad_h16_workspace_floats": (_i64, [_i, _i, _i, _i, _i64]),
    "vatl_conv2d_wgrad_h16": (_i, [_p, _p, _p, _i64] + [_i] * 11 + [_p]),
    "vatl_wgrad_h16_reduce": (_i, [_p, _p, _i64, _i, _i, _i, _i, _i, _p]),
    "vatl_pack_conv_weight_dgrad_h16": (_i, [_p, _p] + [_i] * 7 + [_p]),
    "vatl_conv2d_dgrad_h16": (_i, [_p] * 4 + [_i] * 10 + [_p]),
    "vatl_bn_h16_workspace_doubles": (_i64, [_i64, _i]),
    "vatl_bn_train_fwd_stats_h16": (_i, [_p, _i64, _i, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _i, _p]),
    "vatl_bn_apply_h16": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "vatl_bn_train_bwd_h16": (_i, [_p] * 10 + [_i64, _i, _p, _p, _i, _p]),
    "vatl_maxpool3x3s2_bwd_h16": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "vatl_pack_weights_h16_multi": (_i, [_p, _i, _i64, _i, _p]),
    "vatl_wgrad_f64_splits": (_i64, [_i64]),
    "vatl_conv2d_wgrad_f64_workspace_doubles": (_i64, [_i, _i, _i, _i, _i64]),
    "vatl_conv2d_wgrad_f64": (_i, [_p, _p, _p, _i64] + [_i] * 10 + [_p]),
    "vatl_wgrad_f64_reduce": (_i, [_p, _p, _i64, _i, _i, _i, _i, _i, _p]),
    "vatl_pack_conv_weight_dgrad_f64": (_i, [_p, _p] + [_i] * 6 + [_p]),
    "vatl_conv2d_dgrad_f64": (_i, [_p] * 4 + [_i] * 9 + [_p]),
    "vatl_bn_f64_workspace_doubles": (_i64, [_i64, _i]),
    "vatl_bn_train_fwd_stats_f64": (_i, [_p, _i64, _i, _p, _p, _p, _p, _d, _d, _p, _p, _p]),
    "vatl_bn_apply_f64": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _p]),
    "vatl_bn_train_bwd_f64": (_i, [_p] * 10 + [_i64, _i, _p, _p]),
    "vatl_maxpool3x3s2_bwd_f64": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "vatl_col_sum_f64": (_i, [_p, _i64, _i, _p, _p, _p]),
}

_lib = None


class VatlError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VatlError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(or vatl4pose-wacv2024_amd/build.py). There is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        raise VatlError(f"{what} failed ({rc}): {lib().vatl_last_error().decode()}")


def upload(host, device, dtype=None, owned: bool = False):
    """Host array / CPU tensor -> device tensor WITHOUT draining the stream: staged through PyTorch's pinned-memory cache and copied
    non-blocking.  (A plain `.to(device)` from pageable memory blocks the host until every launch queued before it has finished — a few
    of those per loader batch serialise the host's batch preparation with the device's forward pass.)

    The source is gathered ONCE, straight into a pinned staging buffer of this call (strided views of a loader batch included: no
    pageable intermediate), so the caller may overwrite ``host`` as soon as the call returns — also when ``host`` itself is pinned,
    unless it passes ``owned=True`` ("the buffer is mine and stays untouched until the copy has run": then it is read in place)."""
    t = torch.as_tensor(host)
    device = torch.device(device)
    if t.is_cuda:                                           # already on a device: nothing to stage
        return t.to(device=device, dtype=dtype if dtype is not None else t.dtype)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if device.type != "cuda" or t.numel() == 0:
        return t.to(device)
    if owned and t.is_pinned() and t.is_contiguous():
        return t.to(device, non_blocking=True)
    stage = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)         # caching host allocator: reused once the copy below has completed
    stage.copy_(t)
    return stage.to(device, non_blocking=True)


def _ptr(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise VatlError("vatl_hip needs device (HIP) tensors; there is no CPU path")
    if t.dtype != dtype:
        raise VatlError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise VatlError("tensor must be contiguous")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_tls = _threading.local()                            # per host thread: the plan its pack_* calls consult, the depth of its open splitk_scopes


# ----------------------------------------------------------------------------
# layout
# ----------------------------------------------------------------------------

def nchw_to_nhwc(x: torch.Tensor, cpad: int | None = None) -> torch.Tensor:
    n, c, h, w = x.shape
    cpad = cpad or c
    y = torch.empty((n, h, w, cpad), device=x.device, dtype=torch.float32)
    _check(lib().vatl_nchw_to_nhwc(_ptr(x), _ptr(y), n, c, h, w, cpad, _stream()), "vatl_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    n, h, w, c = x.shape
    y = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
    _check(lib().vatl_nhwc_to_nchw(_ptr(x), _ptr(y), n, c, h, w, _stream()), "vatl_nhwc_to_nchw")
    return y


# ----------------------------------------------------------------------------
# metering, tuning knobs, split-K / stream-K scopes
# ----------------------------------------------------------------------------

ROUTE_NAMES = ("igemm", "igemm_bnbwd", "igemm_dma", "persistent_1x1", "streamk", "rows_1x1", "bottleneck_chain", "stem_pool", "halo_3x3", "winograd",
               "winograd_2h", "winograd_bnbwd", "winograd_persist", "winograd_c32", "wgrad", "winograd_wgrad", "winograd_wgrad_2h", "winograd_wgrad_table", "winograd_f4", "winograd_f4_bnbwd",
               "gemm1x1_ring", "winograd_deconv43", "winograd_s2_43", "stem_pool_w1d", "chain_proj", "chain_step", "gemm1x1_bf16x6",
               "gemm1x1_bf16x6_short")


class flop_meter:
    """`with vh.flop_meter() as fm: ...` — executed MFMA FLOPs (tile padding included) of the matrix-core launches the calling host
    thread makes inside the block: fm.direct (implicit GEMM / weight gradients), fm.winograd (transform-domain GEMMs), fm.total, and the
    launch counts.  Thread-local in the library (vatl_flop_meter_begin / _end); used by bench.py for roofline.frac."""

    def __enter__(self):
        _check(lib().vatl_flop_meter_begin(), "flop_meter_begin")
        self.direct = self.winograd = self.total = 0.0
        self.direct_launches = self.winograd_launches = 0
        return self

    @staticmethod
    def launches_now() -> int:
        """Matrix-core launches metered since __enter__ (every metered launch also bumps exactly one route counter)."""
        counts = (C.c_int64 * len(ROUTE_NAMES))()
        _check(min(0, lib().vatl_flop_meter_routes(counts, len(ROUTE_NAMES))), "flop_meter_routes")
        return int(sum(counts))

    def __exit__(self, *exc):
        counts = (C.c_int64 * len(ROUTE_NAMES))()
        _check(min(0, lib().vatl_flop_meter_routes(counts, len(ROUTE_NAMES))), "flop_meter_routes")
        self.routes = {n: int(c) for n, c in zip(ROUTE_NAMES, counts)}          # launches per kernel family (include/vatl_hip.h VATL_ROUTE_NAMES)
        d, w, nd, nw = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_int64(0)
        _check(lib().vatl_flop_meter_end(C.byref(d), C.byref(w), C.byref(nd), C.byref(nw)), "flop_meter_end")
        self.direct, self.winograd, self.total = d.value, w.value, d.value + w.value
        self.direct_launches, self.winograd_launches = nd.value, nw.value
        return False


def tune_set(knob: int, value: int):
    _check(lib().vatl_tune_set(knob, value), "vatl_tune_set")


_splitk_buf = {}                                     # device index -> workspace tensor kept alive while registered


def enable_splitk(megabytes: int = 64, device=None):
    """Opt-in split-K for small-batch latency on ``device`` (default: the current one; see vatl_set_splitk_workspace);
    ``megabytes = 0`` switches it off for that device."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(idx):                                     # the library files the workspace under the current device
        if megabytes <= 0:
            _check(lib().vatl_set_splitk_workspace(None, 0), "vatl_set_splitk_workspace")
            _splitk_buf.pop(idx, None)
            return
        buf = torch.empty(megabytes * (1 << 18), device=torch.device("cuda", idx), dtype=torch.float32)
        _check(lib().vatl_set_splitk_workspace(_ptr(buf), buf.numel()), "vatl_set_splitk_workspace")
        _splitk_buf[idx] = buf


_splitk_scratch = {}                                 # device index -> free list of workspaces of the automatic small-batch mode
_splitk_scratch_lock = _threading.Lock()
# the batch-invariant cut sizes a layer's split from what a 16-crop batch needs (conv_igemm.hip: launch): the largest is SimplePose's last
# transposed conv, 3 slices x 16 crops x 64 x 48 x 256 floats = 151 MB; a smaller workspace only makes that layer run unsplit
SPLITK_SCRATCH_MB = 256


class splitk_scope:
    """Split-K for the launches of THIS host thread for the duration of one call (the module-call path of small batches,
    alphapose/models/hip_engine.py: run_module_nchw), with the batch-invariant cut, and removed afterwards: the evaluation stream
    — whose crops must have batch-size-independent bits — never sees it, other host threads (DataParallel replicas) are not
    affected and share no buffer with this one.  A device on which split-K was switched on explicitly (``enable_splitk``) is
    left alone.  Workspaces live in a per-DEVICE free list: a scope takes one (allocating only when every buffer of the device
    is in use by another thread's open scope) and puts it back on exit, so a thread-per-call caller does not accumulate buffers."""

    def __init__(self, device, megabytes: int | None = None):
        self.idx = device.index if device.index is not None else torch.cuda.current_device()
        self.mb = megabytes or SPLITK_SCRATCH_MB
        self.active = False
        self.buf = None

    def __enter__(self):
        if self.idx in _splitk_buf:
            return self
        want = self.mb * (1 << 18)
        with _splitk_scratch_lock:
            free = _splitk_scratch.setdefault(self.idx, [])
            hit = next((e for e in free if e[0].numel() >= want), None)
            if hit is not None:
                free.remove(hit)
        if hit is not None:
            self.buf = hit[0]
            torch.cuda.current_stream(self.idx).wait_event(hit[1])      # the previous user's launches (possibly another thread's stream) are done with it
        else:
            self.buf = torch.empty(want, device=torch.device("cuda", self.idx), dtype=torch.float32)
        _check(lib().vatl_set_splitk_workspace_thread(_ptr(self.buf), self.buf.numel()), "vatl_set_splitk_workspace_thread")
        self.active = True
        _tls.latency_mode = getattr(_tls, "latency_mode", 0) + 1
        return self

    def __exit__(self, *exc):
        if self.active:
            _tls.latency_mode -= 1
            _check(lib().vatl_set_splitk_workspace_thread(None, 0), "vatl_set_splitk_workspace_thread")
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.idx))
            with _splitk_scratch_lock:
                _splitk_scratch[self.idx].append((self.buf, ev))
            self.buf = None
            self.active = False
        return False


def latency_mode() -> bool:
    """True inside a ``splitk_scope`` of this host thread: the module-call path of small batches (<= 16 crops).  The inference plans
    then keep every conv on the implicit GEMM, whose split-K fills the chip from a handful of tiles; the Winograd kernels have no
    reduction split (one crop: deconv1 = 32 blocks x 128 serial stages) and are 27 - 40 % slower end to end below ~8 crops."""
    return getattr(_tls, "latency_mode", 0) > 0


STREAMK_IN_TRAINING = False                          # module constant, not an environment switch (see streamk_scope)
_streamk_ws = {}                                     # (host thread, device index) -> zero-initialised stream-K workspace


class streamk_scope:
    """Stream-K for this host thread's conv launches while the scope is open (the trainers' forward / backward passes): launches
    that would leave much of the chip idle share their (tile, k-tile) units evenly over 768 persistent blocks
    (vatl_set_streamk_workspace_thread).  Results are deterministic but not the unsplit kernels' bits, so nothing outside
    training opens it — and the trainers open it only when STREAMK_IN_TRAINING is set (off): measured on MI355X (profiles/r03_notes.md) the route
    gains 8-23 % on the launches it takes when they run ALONE (R50 stage 4 at B = 120, FastPose-R152 stages 3-4 at B = 32), but
    in the real step the block slots those launches leave idle are where the side stream's weight-gradient kernels run, and 768
    persistent blocks take that overlap away: fine-tune step 44.8 -> 44.7 ms (R50), 67.5 -> 70.4 ms (R152).  ``force`` opens it
    regardless (benchmarks, tests)."""

    def __init__(self, device, force: bool = False):
        self.idx = device.index if device.index is not None else torch.cuda.current_device()
        self.active = False
        self.force = force

    def __enter__(self):
        if not self.force and not STREAMK_IN_TRAINING:
            return self
        key = (_threading.get_ident(), self.idx)
        buf = _streamk_ws.get(key)
        if buf is None:
            buf = _streamk_ws[key] = torch.zeros(int(lib().vatl_streamk_workspace_bytes()), device=torch.device("cuda", self.idx), dtype=torch.uint8)
        _check(lib().vatl_set_streamk_workspace_thread(_ptr(buf, torch.uint8), buf.numel()), "vatl_set_streamk_workspace_thread")
        self.active = True
        return self

    def __exit__(self, *exc):
        if self.active:
            _check(lib().vatl_set_streamk_workspace_thread(None, 0), "vatl_set_streamk_workspace_thread")
        return False


# ----------------------------------------------------------------------------
# weight packs and parameter folding
# ----------------------------------------------------------------------------

def conv_cout_pad(cout: int) -> int:
    return lib().vatl_conv_cout_pad(cout)


# VatlPackJob.kind and what the (a, b, c) fields hold for it (include/vatl_hip.h: vatl_pack_weights_multi)
_PACK_CONV = 0                      # conv forward layout, (a, b, c) = (CoutPad, Spad, CinPad)
_PACK_DGRAD = 1                     # data-gradient layout, (a, b, c) = (CinPad, CoutK, ntaps) with the taps in tap_r / tap_s
_PACK_DECONV = 2                    # ConvTranspose2d(4,2,1) layout, src (Cin,Cout,4,4), a = CoutPad
# Winograd F(2x2,3x3) filter transform, forward / data gradient: (Cout, Cin) of the PACKED filter, a = its padded Cout, b = 32-channel groups per
# tile (a / 32 <= 1 ? 1 : 2), c = Cin (kind 3) or Cout (kind 4) = the inner dimension of src
_PACK_WINOGRAD = 3
_PACK_WINOGRAD_DGRAD = 4
_PACK_WINOGRAD_DECONV = 5           # Winograd F(3x3,2x2) phase filters of ConvTranspose2d(4,2,1): src (Cin,Cout,4,4), a / b as for kinds 3 / 4, c = Cout
_PACK_WINOGRAD_DECONV_DGRAD = 6     # the filters of its data gradient: (Cout, Cin) fields = (layer Cin, layer Cout), c = layer Cout
_PACK_WINOGRAD_F4 = 7               # Winograd F(4x4,3x3) filter transform, forward: (Cout, Cin) of the PACKED filter, c = inner dimension of src
_PACK_WINOGRAD_F4_DGRAD = 8         # ... data gradient


class _PackJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("first_block", C.c_int64), ("kind", C.c_int32), ("Cout", C.c_int32), ("Cin", C.c_int32),
                ("R", C.c_int32), ("S", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("tap_r", C.c_int32 * 16), ("tap_s", C.c_int32 * 16)]


class PackPlan:
    """The weight re-packs of one fine-tune step as ONE launch (vatl_pack_weights_multi).

    The trainers (alphapose/models/hip_train.py) ask for packed copies through ``pack_conv_weight`` / ``pack_deconv_weight`` /
    ``pack_dgrad_weight`` where they need them.  The first step under a plan runs those calls as usual and RECORDS them (source
    tensor, layout, destination buffer, which is then kept); ``seal()`` uploads the descriptor table.  From the next step on,
    ``begin()`` refreshes every recorded destination with one launch and the pack calls return the kept buffers.  A lookup is
    honoured only if the source tensor is the recorded storage at the version it had at ``begin()`` (optimizers that write
    through the C ABI bump the version counters): anything else is packed on the spot, and makes the plan re-record."""

    def __init__(self):
        self.jobs = {}            # key -> [src tensor, dst tensor, descriptor fields, version at begin()]
        self.table = None
        self.total_blocks = 0
        self.ready = False
        self.stale = False

    def begin(self):
        if self.ready and not self.stale:
            for j in self.jobs.values():
                j[3] = j[0]._version
            _check(lib().vatl_pack_weights_multi(_ptr(self.table, torch.uint8), len(self.jobs), self.total_blocks, _stream()), "vatl_pack_weights_multi")
        else:
            self.jobs, self.table, self.ready, self.stale = {}, None, False, False

    def lookup(self, key, w):
        if not self.ready:
            return None
        j = self.jobs.get(key)
        if j is None or j[0].data_ptr() != w.data_ptr() or j[3] != w._version:
            self.stale = True                      # a layout the recording did not see, or weights that changed since begin()
            return None
        return j[1]

    def record(self, key, w, dst, fields):
        if not self.ready and key not in self.jobs:
            self.jobs[key] = [w, dst, fields, w._version]

    def seal(self):
        if self.ready or not self.jobs:
            return
        arr = (_PackJob * len(self.jobs))()
        blocks = 0
        for k, (src, dst, f, _) in enumerate(self.jobs.values()):
            jb = arr[k]
            jb.src, jb.dst, jb.first_block = src.data_ptr(), dst.data_ptr(), blocks
            jb.kind, jb.Cout, jb.Cin, jb.R, jb.S, jb.a, jb.b, jb.c = f[:8]
            for t, (tr, ts) in enumerate(f[8]):
                jb.tap_r[t], jb.tap_s[t] = tr, ts
            if f[0] == _PACK_DGRAD:                          # [a = CinPad][c = taps][b = CoutK]: 32 x 32 tiles of one tap
                blocks += ((f[5] + 31) // 32) * f[7] * ((f[6] + 31) // 32)
            elif f[0] in (_PACK_WINOGRAD, _PACK_WINOGRAD_DGRAD, _PACK_WINOGRAD_DECONV, _PACK_WINOGRAD_DECONV_DGRAD):
                blocks += dst.numel() // 4096                # F(2x2) / F(3x3,2x2) Winograd filters: 4096 elements per block
            else:
                blocks += (dst.numel() + 1023) // 1024       # everything else 1024
        dev = next(iter(self.jobs.values()))[1].device
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table = host.to(dev)
        self.total_blocks = blocks
        self.ready = True


def set_pack_plan(plan):
    """The plan the pack_* calls of THIS host thread consult (None: every call packs on the spot).  Returns the previous one."""
    prev = getattr(_tls, "pack_plan", None)
    _tls.pack_plan = plan
    return prev


def _pack(key, w, job, planned: bool = True):
    """What every plan-aware pack_* wrapper does around its one launch.  When the PackPlan of this host thread (set_pack_plan) keeps
    a buffer for ``key`` that is current for ``w``, that buffer is the result.  Otherwise ``job()`` says what to run: (shape of the
    packed tensor, C entry point, its arguments between (src, dst) and the stream, the VatlPackJob fields (kind, Cout, Cin, R, S,
    a, b, c, taps)) — allocate, launch, and let the plan record the job.  A non-contiguous ``w`` is packed from a contiguous copy and
    stays outside the plan (the plan's one launch reads the parameter's own storage)."""
    plan = getattr(_tls, "pack_plan", None) if planned and w.is_contiguous() else None
    if plan is not None:
        kept = plan.lookup(key, w)
        if kept is not None:
            return kept
    shape, fn, args, fields = job()
    out = torch.empty(shape, device=w.device, dtype=torch.float32)
    _check(getattr(lib(), fn)(_ptr(w.contiguous()), _ptr(out), *args, _stream()), fn)
    if plan is not None:
        plan.record(key, w, out, fields)
    return out


def _winograd_fields(kind: int, cout: int, cin: int, k: int, inner: int):
    """VatlPackJob fields of the F(2x2,3x3) / F(3x3,2x2) filter transforms (kinds 3 .. 6)."""
    pad = int(lib().vatl_winograd_cout_pad(cout))
    return (kind, cout, cin, k, k, pad, 1 if pad <= 32 else 2, inner, ())


def pack_conv_weight(w: torch.Tensor, planned: bool = True) -> torch.Tensor:
    """(Cout,Cin,R,S) -> [CoutPad][R][Spad][CinPad]; the 3-channel stem is padded to 4 channels x 8 taps.  ``planned=False`` keeps the
    call out of the thread's PackPlan (a source that is a temporary, not a parameter)."""
    cout, cin, r, s = w.shape
    cpad = conv_cout_pad(cout)
    if r == 1 and s == 1 and cpad == cout and cin != 3 and w.is_contiguous() and w.dtype == torch.float32:
        return w.detach().view(cout, 1, 1, cin)              # (Cout,Cin,1,1) already is the packed [Cout][1][1][Cin]: no copy
    spad, cinpad = (8, 4) if cin == 3 else (s, cin)
    return _pack(("conv", w.data_ptr(), tuple(w.shape)), w, lambda: (
        (cpad, r, spad, cinpad), "vatl_pack_conv_weight", (cout, cin, r, s, cpad, spad, cinpad),
        (_PACK_CONV, cout, cin, r, s, cpad, spad, cinpad, ())), planned=planned)


def pack_dgrad_weight(w: torch.Tensor, taps, cout_k: int | None = None, planned: bool = True) -> torch.Tensor:
    """(Cout,Cin,R,S) -> [CinPad][len(taps)][CoutK] with out[c][t][n] = w[n][c][taps[t]]."""
    cout, cin, r, s = w.shape
    cinpad = conv_cout_pad(cin)
    cout_k = cout_k or cout
    taps = [(int(a), int(b)) for a, b in taps]

    def job():
        tr = (C.c_int * len(taps))(*[t[0] for t in taps])
        ts = (C.c_int * len(taps))(*[t[1] for t in taps])
        return ((cinpad, len(taps), cout_k), "vatl_pack_dgrad_weight",
                (cout, cin, r, s, cinpad, cout_k, len(taps), C.cast(tr, C.c_void_p), C.cast(ts, C.c_void_p)),
                (_PACK_DGRAD, cout, cin, r, s, cinpad, cout_k, len(taps), tuple(taps)))
    return _pack(("dgrad", w.data_ptr(), tuple(w.shape), tuple(taps), cout_k), w, job, planned=planned and len(taps) <= 16)     # VatlPackJob holds 16 taps


def pack_deconv_weight(w: torch.Tensor) -> torch.Tensor:
    cin, cout, kh, kw = w.shape
    if (kh, kw) != (4, 4):
        raise VatlError("only ConvTranspose2d(4, 2, 1) is supported")
    cpad = conv_cout_pad(cout)
    return _pack(("deconv", w.data_ptr(), tuple(w.shape)), w, lambda: (
        (4, cpad, 2, 2, cin), "vatl_pack_deconv4x4s2_weight", (cin, cout, cpad), (_PACK_DECONV, cout, cin, 4, 4, cpad, 0, 0, ())))


def pack_winograd_weight(w: torch.Tensor, data_gradient: bool = False) -> torch.Tensor:
    """(Cout,Cin,3,3) -> the F(2x2,3x3) filter transform G g G^T in MFMA fragment order (csrc/conv_winograd.hip).  With
    ``data_gradient`` the result is the filter of dX = conv(dY, rot180(w)^T): its output channels are the forward Cin."""
    co, ci = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3):
        raise VatlError("pack_winograd_weight: 3x3 filters only")
    cout, cin = (ci, co) if data_gradient else (co, ci)
    return _pack(("winograd", w.data_ptr(), tuple(w.shape), bool(data_gradient)), w, lambda: (
        int(lib().vatl_winograd_weight_floats(cout, cin)), "vatl_pack_winograd_weight", (cout, cin, int(data_gradient)),
        _winograd_fields(_PACK_WINOGRAD_DGRAD if data_gradient else _PACK_WINOGRAD, cout, cin, 3, ci)))


def pack_winograd_f4_weight(w: torch.Tensor, data_gradient: bool = False) -> torch.Tensor:
    """(Cout,Cin,3,3) -> U = G g G^T of F(4x4,3x3) in the MFMA fragment order of csrc/winograd_f4.hip.  With ``data_gradient`` the result is the filter of
    dX = conv(dY, rot180(w)^T): its output channels are the forward Cin.  Inside a PackPlan (the trainers' forward / backward) the buffer is kept and refreshed by
    the step's one re-pack launch."""
    co, ci = w.shape[:2]
    cout, cin = (ci, co) if data_gradient else (co, ci)
    return _pack(("winograd_f4", w.data_ptr(), tuple(w.shape), bool(data_gradient)), w, lambda: (
        int(lib().vatl_winograd_f4_weight_floats(cout, cin)), "vatl_pack_winograd_f4_weight", (cout, cin, int(data_gradient)),
        (_PACK_WINOGRAD_F4_DGRAD if data_gradient else _PACK_WINOGRAD_F4, cout, cin, 3, 3, 0, 0, ci, ())))


def pack_winograd_deconv_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) -> the four sub-pixel phase filters in the F(3x3,2x2) transform domain,
    MFMA fragment order (csrc/conv_winograd.hip)."""
    cin, cout = w.shape[:2]
    if tuple(w.shape[2:]) != (4, 4):
        raise VatlError("pack_winograd_deconv_weight: 4x4 filters only")
    return _pack(("winograd_deconv", w.data_ptr(), tuple(w.shape)), w, lambda: (
        int(lib().vatl_winograd_deconv_weight_floats(cout, cin)), "vatl_pack_winograd_deconv_weight", (cout, cin),
        _winograd_fields(_PACK_WINOGRAD_DECONV, cout, cin, 4, cout)))


def pack_winograd_deconv43_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) -> the four phase filters in the F(4x3,2x2) transform domain, 20 positions each, MFMA fragment
    order (csrc/winograd_deconv43.hip).  Inference only: packed on the spot, never part of a PackPlan's one-launch re-pack table."""
    cin, cout = w.shape[:2]
    if tuple(w.shape[2:]) != (4, 4):
        raise VatlError("pack_winograd_deconv43_weight: 4x4 filters only")
    return _pack(("winograd_deconv43", w.data_ptr(), tuple(w.shape)), w, lambda: (
        int(lib().vatl_winograd_deconv43_weight_floats(cout, cin)), "vatl_pack_winograd_deconv43_weight", (cout, cin), None), planned=False)


def pack_winograd_s2_43_weight(w: torch.Tensor) -> torch.Tensor:
    """3x3 / stride 2 / pad 1 conv weight (Cout,Cin,3,3) -> its four input-phase filters in the F(4x3,2x2) transform domain (20 positions for the two
    by = 0 phases, 16 for the two by = 1), concatenated along the step index in MFMA fragment order (csrc/winograd_s2_43.hip).  Inference only: packed on
    the spot, never part of a PackPlan's one-launch re-pack table."""
    cout, cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3):
        raise VatlError("pack_winograd_s2_43_weight: 3x3 filters only")
    return _pack(("winograd_s2_43", w.data_ptr(), tuple(w.shape)), w, lambda: (
        int(lib().vatl_winograd_s2_43_weight_floats(cout, cin)), "vatl_pack_winograd_s2_43_weight", (cout, cin), None), planned=False)


def pack_gemm1x1_bf16x6_weight(w: torch.Tensor) -> torch.Tensor:
    """The [N][K] fp32 filter of a 1x1 layer (pack_conv_weight's (N,1,1,K), or the rows of pack_conv1x1_dual_weight) -> its three bf16 planes (csrc/split16.h) in
    the order the B fragments of csrc/gemm1x1_bf16x6.hip are read: 6 bytes per weight.  Inference only: packed on the spot, never part of a PackPlan's
    one-launch re-pack table."""
    n = w.shape[0]
    k = w.numel() // n
    return _pack(("gemm1x1_bf16x6", w.data_ptr(), tuple(w.shape)), w, lambda: (
        int(lib().vatl_gemm1x1_bf16x6_weight_floats(n, k)), "vatl_pack_gemm1x1_bf16x6_weight", (n, k), None), planned=False)


def pack_winograd_deconv_dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) -> the filters of its DATA gradient (a 4x4 / stride 2 conv over dz = four pixel
    phases x 2x2 convolutions) in the F(3x3,2x2) transform domain."""
    cin, cout = w.shape[:2]
    if tuple(w.shape[2:]) != (4, 4):
        raise VatlError("pack_winograd_deconv_dgrad_weight: 4x4 filters only")
    return _pack(("winograd_deconv_dgrad", w.data_ptr(), tuple(w.shape)), w, lambda: (
        int(lib().vatl_winograd_deconv_dgrad_weight_floats(cin, cout)), "vatl_pack_winograd_deconv_dgrad_weight", (cin, cout),
        _winograd_fields(_PACK_WINOGRAD_DECONV_DGRAD, cin, cout, 4, cout)))


def pack_conv1x1_dual_weight(w1, scale1, bias1, w2, scale2, bias2):
    """Two (Cout,C,1,1) weights + folded BN scale/bias -> ([CoutPad][C1+C2] scaled rows, bias1 + bias2)."""
    cout, c1 = w1.shape[:2]
    c2 = w2.shape[1]
    cpad = conv_cout_pad(cout)
    out = torch.empty((cpad, c1 + c2), device=w1.device, dtype=torch.float32)
    bias = torch.empty(cout, device=w1.device, dtype=torch.float32)
    _check(lib().vatl_pack_conv1x1_dual_weight(_ptr(w1.contiguous()), _ptr(scale1), _ptr(bias1), _ptr(w2.contiguous()), _ptr(scale2), _ptr(bias2),
                                               _ptr(out), _ptr(bias), cout, c1, c2, cpad, _stream()), "vatl_pack_conv1x1_dual_weight")
    return out, bias


def pack_winograd_c32_weight(w: torch.Tensor) -> torch.Tensor:
    """(32,32,3,3) -> G g G^T in the LDS order of csrc/winograd_c32.hip."""
    if tuple(w.shape) != (32, 32, 3, 3):
        raise VatlError("pack_winograd_c32_weight: a (32, 32, 3, 3) filter")
    out = torch.empty(int(lib().vatl_winograd_c32_weight_floats()), device=w.device, dtype=torch.float32)
    _check(lib().vatl_pack_winograd_c32_weight(_ptr(w.contiguous()), _ptr(out), _stream()), "vatl_pack_winograd_c32_weight")
    return out


def pack_stem_pool_weight(w: torch.Tensor) -> torch.Tensor:
    """(64,3,7,7) OIHW stem filter -> the fragment order of vatl_stem7x7s2_pool_fwd."""
    if tuple(w.shape) != (64, 3, 7, 7):
        raise VatlError(f"pack_stem_pool_weight: expected a (64,3,7,7) filter, got {tuple(w.shape)}")
    w = w.detach().float().contiguous()
    out = torch.empty(int(lib().vatl_stem_pool_weight_floats()), device=w.device, dtype=torch.float32)
    _check(lib().vatl_pack_stem_pool_weight(_ptr(w), _ptr(out), _stream()), "vatl_pack_stem_pool_weight")
    return out


def pack_stem_pool_w1d_weight(w: torch.Tensor) -> torch.Tensor:
    """(64,3,7,7) OIHW stem filter -> its 1-D Winograd transform in the fragment order of vatl_stem7x7s2_pool_w1d_fwd (csrc/stem_pool_w1d.hip): positions 0 - 4 =
    G4 w[..., 0::2], 5 - 8 = G3 w[..., 1::2], float64 rounded once.  Inference only: packed on the spot, never part of a PackPlan's one-launch re-pack table."""
    if tuple(w.shape) != (64, 3, 7, 7):
        raise VatlError(f"pack_stem_pool_w1d_weight: expected a (64,3,7,7) filter, got {tuple(w.shape)}")
    w = w.detach().float().contiguous()
    out = torch.empty(int(lib().vatl_stem_pool_w1d_weight_floats()), device=w.device, dtype=torch.float32)
    _check(lib().vatl_pack_stem_pool_w1d_weight(_ptr(w), _ptr(out), _stream()), "vatl_pack_stem_pool_w1d_weight")
    return out


def pack_stem3_weight(w: torch.Tensor) -> torch.Tensor:
    """(64,3,3,3) OIHW filter of HRNet's conv1 -> the fragment order of vatl_stem3x3s2_fwd."""
    if tuple(w.shape) != (64, 3, 3, 3):
        raise VatlError(f"pack_stem3_weight: expected a (64,3,3,3) filter, got {tuple(w.shape)}")
    w = w.detach().float().contiguous()
    out = torch.empty(int(lib().vatl_stem3_weight_floats()), device=w.device, dtype=torch.float32)
    _check(lib().vatl_pack_stem3_weight(_ptr(w), _ptr(out), _stream()), "vatl_pack_stem3_weight")
    return out


def bn_fold(gamma, beta, mean, var, eps: float, conv_bias=None, channels: int | None = None):
    c = channels if channels is not None else (var.numel() if var is not None else conv_bias.numel())
    dev = (var if var is not None else conv_bias).device
    scale = torch.empty(c, device=dev, dtype=torch.float32)
    bias = torch.empty(c, device=dev, dtype=torch.float32)
    _check(lib().vatl_bn_fold(_ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), _ptr(conv_bias), eps, _ptr(scale), _ptr(bias), c, _stream()), "vatl_bn_fold")
    return scale, bias


# ----------------------------------------------------------------------------
# backbone ops (NHWC)
# ----------------------------------------------------------------------------

def conv3x3s2_winograd43_supported(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    return bool(lib().vatl_conv3x3s2_winograd43_supported(n, h, w, cin, cout))


def gemm1x1_bf16x6_supported(m: int, k: int, k1: int, n: int) -> bool:
    """m rows of a 1x1 / stride-1 layer k -> n (k1 = 0), or of the dual form (k1 + (k - k1)) -> n, on the bf16x6 GEMM (csrc/gemm1x1_bf16x6.hip)."""
    return bool(lib().vatl_gemm1x1_bf16x6_supported(m, k, k1, n))


def gemm1x1_bf16x6_short_supported(m: int, k: int, n: int) -> bool:
    """m rows of a 1x1 / stride-1 layer k -> n on the short-K form of the bf16x6 GEMM (128 <= k < 512, k % 64 == 0, n >= 512, n % 256 == 0; conv1x1_rows_fwd(..., u_x6=))."""
    return bool(lib().vatl_gemm1x1_bf16x6_short_supported(m, k, n))


def conv2d_fwd(x, w_packed, scale, bias, cout: int, r: int, s: int, stride: int, pad: int, relu: bool,
               residual=None, out_nchw: bool = False, out=None, u_s2=None, u_x6=None):
    """Conv2d + folded BN (+ residual) (+ ReLU) of an NHWC tensor on the implicit GEMM — or, when ``u_s2`` (pack_winograd_s2_43_weight) is given and the
    call is a 3x3 / stride 2 / pad 1 layer without residual, NHWC output, of a shape the kernel serves (conv3x3s2_winograd43_supported), as Winograd
    F(4x3,2x2) summed over the four input phases (csrc/winograd_s2_43.hip; other bits).  Every other call ignores ``u_s2``.
    With ``u_x6`` (pack_gemm1x1_bf16x6_weight) a 1x1 / stride 1 layer with NHWC output of a shape gemm1x1_bf16x6_supported admits runs as six bf16 MFMAs per
    product (csrc/gemm1x1_bf16x6.hip; same values to fp32 rounding, other bits); every other call ignores ``u_x6``."""
    n, h, w, cin = x.shape
    ho = (h + 2 * pad - r) // stride + 1
    wo = (w + 2 * pad - s) // stride + 1
    shape = (n, cout, ho, wo) if out_nchw else (n, ho, wo, cout)
    y = out if out is not None else torch.empty(shape, device=x.device, dtype=torch.float32)
    if (u_s2 is not None and (r, s, stride, pad) == (3, 3, 2, 1) and residual is None and not out_nchw
            and conv3x3s2_winograd43_supported(n, h, w, cin, cout)):
        _check(lib().vatl_conv3x3s2_winograd43_fwd(_ptr(x), _ptr(u_s2), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, cin, cout, int(relu), _stream()),
               "vatl_conv3x3s2_winograd43_fwd")
        return y
    if u_x6 is not None and (r, s, stride, pad) == (1, 1, 1, 0) and not out_nchw and gemm1x1_bf16x6_supported(n * h * w, cin, 0, cout):
        _check(lib().vatl_gemm1x1_bf16x6_fwd(_ptr(x), _ptr(u_x6), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, cin, cout, stride, int(relu),
                                             _stream()), "vatl_gemm1x1_bf16x6_fwd")
        return y
    _check(lib().vatl_conv2d_fwd(_ptr(x), _ptr(w_packed), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, cin, cout,
                                 w_packed.shape[0], r, s, stride, pad, int(relu), int(out_nchw), _stream()), "vatl_conv2d_fwd")
    return y


def conv1x1_dual_fwd(a, x, w_packed, bias, cout: int, stride2: int, relu: bool, out=None, u_x6=None):
    """relu?(W1' a + W2' x[::s, ::s] + bias): a (N,Ho,Wo,C1) and x (N,H2,W2,C2) NHWC -> (N,Ho,Wo,Cout).  With ``u_x6`` (pack_gemm1x1_bf16x6_weight of
    w_packed) and a shape gemm1x1_bf16x6_supported admits, as six bf16 MFMAs per product (csrc/gemm1x1_bf16x6.hip; other bits); else ``u_x6`` is ignored."""
    n, ho, wo, c1 = a.shape
    _, h2, w2, c2 = x.shape
    y = out if out is not None else torch.empty((n, ho, wo, cout), device=a.device, dtype=torch.float32)
    if u_x6 is not None and gemm1x1_bf16x6_supported(n * ho * wo, c1 + c2, c1, cout):
        _check(lib().vatl_gemm1x1_bf16x6_dual_fwd(_ptr(a), _ptr(x), _ptr(u_x6), _ptr(bias), None, _ptr(y), n, ho, wo, c1, h2, w2, c2, stride2, cout, int(relu),
                                                  _stream()), "vatl_gemm1x1_bf16x6_dual_fwd")
        return y
    _check(lib().vatl_conv1x1_dual_fwd(_ptr(a), _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(y), n, ho, wo, c1, h2, w2, c2, stride2, cout,
                                       w_packed.shape[0], int(relu), _stream()), "vatl_conv1x1_dual_fwd")
    return y


def conv1x1_rows_supported(k1: int, k2: int, n: int, m: int) -> bool:
    return bool(lib().vatl_conv1x1_rows_supported(k1, k2, n, m))


def conv1x1_rows_fwd(a, w, scale, bias, cout: int, relu: bool, residual=None, x2=None, out=None, next_conv1=None, y1_out=None, u_x6=None):
    """relu?(scale * (A W^T) + bias + residual) for K = 128 input channels (a (N,H,W,128), or a (N,H,W,64) + x2 (N,H,W,64)); w [cout][128] packed.
    next_conv1 = (w1, scale1, bias1) of the next block's 256 -> 64 conv1 (two-source form only): the same launch also computes
    y1 = relu(scale1 * (y W1^T) + bias1) from the tile in LDS (vatl_chain_proj_fwd) and the call returns (y, y1).
    With ``u_x6`` (pack_gemm1x1_bf16x6_weight of w) a single-source call of a shape gemm1x1_bf16x6_short_supported admits runs as six bf16 MFMAs per
    product (csrc/gemm1x1_bf16x6.hip, the short-K form; same values to fp32 rounding, other bits); every other call ignores ``u_x6``."""
    n, h, w_, k1 = a.shape
    k2 = 0 if x2 is None else x2.shape[-1]
    assert w.numel() >= cout * (k1 + k2) and (x2 is None or tuple(x2.shape[:3]) == (n, h, w_)) and (residual is None or tuple(residual.shape) == (n, h, w_, cout))
    y = out if out is not None else torch.empty((n, h, w_, cout), device=a.device, dtype=torch.float32)
    assert a.is_contiguous() and y.is_contiguous() and (x2 is None or x2.is_contiguous()) and (residual is None or residual.is_contiguous())
    if next_conv1 is not None:
        w1, scale1, bias1 = next_conv1
        cnext = w1.shape[0]
        if x2 is None or k2 != k1 or residual is not None:
            raise VatlError("conv1x1_rows_fwd: next_conv1 goes with the two-source form (a, x2 of 64 channels each) and no residual")
        assert w1.numel() == cnext * cout
        y1 = y1_out if y1_out is not None else torch.empty((n, h, w_, cnext), device=a.device, dtype=torch.float32)
        assert y1.is_contiguous()
        _check(lib().vatl_chain_proj_fwd(_ptr(a), _ptr(x2), _ptr(w), _ptr(scale), _ptr(bias), _ptr(y), _ptr(w1), _ptr(scale1), _ptr(bias1), _ptr(y1),
                                         n * h * w_, k1, cout, cnext, int(relu), _stream()), "vatl_chain_proj_fwd")
        return y, y1
    if u_x6 is not None and x2 is None and gemm1x1_bf16x6_short_supported(n * h * w_, k1, cout):
        _check(lib().vatl_gemm1x1_bf16x6_short_fwd(_ptr(a), _ptr(u_x6), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n, h, w_, k1, cout, 1, int(relu),
                                                   _stream()), "vatl_gemm1x1_bf16x6_short_fwd")
        return y
    _check(lib().vatl_conv1x1_rows_fwd(_ptr(a), _ptr(x2), _ptr(w), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n * h * w_, k1, k2, cout, int(relu),
                                       _stream()), "vatl_conv1x1_rows_fwd")
    return y


def bottleneck_chain_supported(cmid: int, cout: int, cnext: int, m: int) -> bool:
    return bool(lib().vatl_bottleneck_chain_supported(cmid, cout, cnext, m))


def chain_proj_supported(cmid: int, cout: int, cnext: int, m: int) -> bool:
    """conv3 + projection of a stage's first block with the next block's conv1 (conv1x1_rows_fwd(..., next_conv1=)): 64 + 64 -> 256 -> 64."""
    return bool(lib().vatl_chain_proj_supported(cmid, cout, cnext, m))


def chain_step_supported(cmid: int, cout: int, cnext: int, m: int) -> bool:
    """conv3 + skip of a stage's last block with the next stage's first conv1 (bottleneck_chain_fwd(..., next_stage_conv1=)): 64 -> 256 -> 128."""
    return bool(lib().vatl_chain_step_supported(cmid, cout, cnext, m))


def bottleneck_chain_fwd(a, w3, scale3, bias3, skip, w1=None, scale1=None, bias1=None, out=None, y1_out=None, next_stage_conv1=None):
    """t = relu(bn3(conv3(a)) + skip) and, when w1 is given, y1 = relu(bn1(conv1_next(t))) in one launch: a (N,H,W,Cmid), skip (N,H,W,Cout) NHWC,
    w3 / w1 = packed 1x1 filters (pack_conv_weight).  Returns (t, y1) (y1 None without w1).
    next_stage_conv1 = (w1, scale1, bias1) of a 256 -> 128 conv1 (the first block of the next stage; not together with w1): the same, through
    vatl_chain_step_fwd (y1 has the bits of conv1x1_rows_fwd)."""
    n, h, w_, cmid = a.shape
    cout = w3.shape[0]
    step = next_stage_conv1 is not None
    if step:
        if w1 is not None:
            raise VatlError("bottleneck_chain_fwd: w1 and next_stage_conv1 are exclusive")
        w1, scale1, bias1 = next_stage_conv1
    cnext = 0 if w1 is None else w1.shape[0]
    assert w3.numel() == cout * cmid and (w1 is None or w1.numel() == cnext * cout) and (skip is None or tuple(skip.shape) == (n, h, w_, cout))
    t = out if out is not None else torch.empty((n, h, w_, cout), device=a.device, dtype=torch.float32)
    assert t.is_contiguous() and a.is_contiguous() and (skip is None or skip.is_contiguous())
    y1 = None if w1 is None else (y1_out if y1_out is not None else torch.empty((n, h, w_, cnext), device=a.device, dtype=torch.float32))
    assert y1 is None or y1.is_contiguous()
    fn, name = (lib().vatl_chain_step_fwd, "vatl_chain_step_fwd") if step else (lib().vatl_bottleneck_chain_fwd, "vatl_bottleneck_chain_fwd")
    _check(fn(_ptr(a), _ptr(w3), _ptr(scale3), _ptr(bias3), _ptr(skip), _ptr(t), _ptr(w1), _ptr(scale1), _ptr(bias1), _ptr(y1),
              n * h * w_, cmid, cout, cnext, _stream()), name)
    return t, y1


def stem3_fwd(x_nchw: torch.Tensor, w_packed: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, out=None) -> torch.Tensor:
    """NCHW crops (N,3,H,W) -> conv3x3/2 + folded BN + ReLU -> NHWC (N,H/2,W/2,64) in one launch (hrnet.py:109-110, 426-428)."""
    n, c, h, w = x_nchw.shape
    if c != 3:
        raise VatlError(f"stem3_fwd: expected 3 input channels, got {c}")
    y = out if out is not None else torch.empty((n, h // 2, w // 2, 64), device=x_nchw.device, dtype=torch.float32)
    _check(lib().vatl_stem3x3s2_fwd(_ptr(x_nchw), _ptr(w_packed), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, _stream()), "vatl_stem3x3s2_fwd")
    return y


def stem_pool_supported(h: int, w: int) -> bool:
    return bool(lib().vatl_stem_pool_supported(int(h), int(w)))


def stem_pool_w1d_supported(h: int, w: int) -> bool:
    return bool(lib().vatl_stem_pool_w1d_supported(int(h), int(w)))


def stem_pool_w1d_fwd(x_nchw: torch.Tensor, u1d: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, out=None) -> torch.Tensor:
    """stem_pool_fwd on the 1-D Winograd kernel alone (csrc/stem_pool_w1d.hip); a size it does not serve is an error."""
    n, c, h, w = x_nchw.shape
    if c != 3:
        raise VatlError(f"stem_pool_w1d_fwd: expected 3 input channels, got {c}")
    y = out if out is not None else torch.empty((n, h // 4, w // 4, 64), device=x_nchw.device, dtype=torch.float32)
    _check(lib().vatl_stem7x7s2_pool_w1d_fwd(_ptr(x_nchw), _ptr(u1d), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, _stream()), "vatl_stem7x7s2_pool_w1d_fwd")
    return y


def stem_pool_fwd(x_nchw: torch.Tensor, w_packed: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, out=None, u1d=None) -> torch.Tensor:
    """NCHW crops (N,3,H,W) -> conv7x7/2 + folded BN + ReLU + maxpool3x3/2 -> NHWC (N,H/4,W/4,64) in one launch (Resnet.py:155-158, 171-172).  With ``u1d``
    (pack_stem_pool_w1d_weight) and a size that kernel serves (stem_pool_w1d_supported) the launch is the 1-D Winograd stem (csrc/stem_pool_w1d.hip; other
    bits); every other call ignores ``u1d``."""
    n, c, h, w = x_nchw.shape
    if c != 3:
        raise VatlError(f"stem_pool_fwd: expected 3 input channels, got {c}")
    y = out if out is not None else torch.empty((n, h // 4, w // 4, 64), device=x_nchw.device, dtype=torch.float32)
    if u1d is not None and stem_pool_w1d_supported(h, w):
        _check(lib().vatl_stem7x7s2_pool_w1d_fwd(_ptr(x_nchw), _ptr(u1d), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, _stream()), "vatl_stem7x7s2_pool_w1d_fwd")
        return y
    _check(lib().vatl_stem7x7s2_pool_fwd(_ptr(x_nchw), _ptr(w_packed), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, _stream()), "vatl_stem7x7s2_pool_fwd")
    return y


def conv3x3_winograd_fwd(x, u_packed, scale, bias, cout: int, relu: bool, residual=None, out=None):
    """3x3 / stride 1 / pad 1 convolution of an NHWC tensor through Winograd F(2x2, 3x3)."""
    n, h, w, cin = x.shape
    y = out if out is not None else torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    _check(lib().vatl_conv3x3_winograd_fwd(_ptr(x), _ptr(u_packed), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, cin, cout,
                                           int(relu), _stream()), "vatl_conv3x3_winograd_fwd")
    return y


def conv3x3_winograd_c32_supported(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    return bool(lib().vatl_conv3x3_winograd_c32_supported(n, h, w, cin, cout))


def conv3x3_winograd_c32_fwd(x, u, scale, bias, relu: bool, residual=None, out=None):
    """3x3 / stride 1 / pad 1, 32 -> 32 channels, NHWC, Winograd F(2x2,3x3) with wave-private tiles (csrc/winograd_c32.hip)."""
    n, h, w, c = x.shape
    y = out if out is not None else torch.empty_like(x)
    assert x.is_contiguous() and y.is_contiguous() and (residual is None or (residual.is_contiguous() and residual.shape == x.shape))
    _check(lib().vatl_conv3x3_winograd_c32_fwd(_ptr(x), _ptr(u), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, int(relu), _stream()),
           "vatl_conv3x3_winograd_c32_fwd")
    return y


def conv3x3_winograd_f4_supported(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    return bool(lib().vatl_conv3x3_winograd_f4_supported(n, h, w, cin, cout))


def conv3x3_winograd_f4_fwd(x, u, scale, bias, cout: int, relu: bool, residual=None, out=None):
    """3x3 / stride 1 / pad 1 conv as Winograd F(4x4,3x3): x NHWC (N,H,W,Cin), H and W multiples of 4 -> (N,H,W,Cout)."""
    n, h, w, cin = x.shape
    y = out if out is not None else torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    _check(lib().vatl_conv3x3_winograd_f4_fwd(_ptr(x), _ptr(u), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, cin, cout, int(relu), _stream()),
           "vatl_conv3x3_winograd_f4_fwd")
    return y


def deconv4x4s2_fwd(x, w_packed, scale, bias, cout: int, relu: bool):
    n, h, w, cin = x.shape
    y = torch.empty((n, 2 * h, 2 * w, cout), device=x.device, dtype=torch.float32)
    _check(lib().vatl_deconv4x4s2_fwd(_ptr(x), _ptr(w_packed), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, cin, cout,
                                      w_packed.shape[1], int(relu), _stream()), "vatl_deconv4x4s2_fwd")
    return y


def deconv4x4s2_winograd43_supported(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    return bool(lib().vatl_deconv4x4s2_winograd43_supported(n, h, w, cin, cout))


def deconv4x4s2_winograd_fwd(x, u_packed, scale, bias, cout: int, relu: bool, out=None, u43=None):
    """ConvTranspose2d(4,2,1) of an NHWC tensor through Winograd F(3x3, 2x2) on its four sub-pixel phases — or, when ``u43``
    (pack_winograd_deconv43_weight) is given and the shape is one the F(4x3, 2x2) kernel serves, through that kernel (other bits)."""
    n, h, w, cin = x.shape
    y = out if out is not None else torch.empty((n, 2 * h, 2 * w, cout), device=x.device, dtype=torch.float32)
    if u43 is not None and deconv4x4s2_winograd43_supported(n, h, w, cin, cout):
        _check(lib().vatl_deconv4x4s2_winograd43_fwd(_ptr(x), _ptr(u43), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, cin, cout, int(relu), _stream()),
               "vatl_deconv4x4s2_winograd43_fwd")
        return y
    _check(lib().vatl_deconv4x4s2_winograd_fwd(_ptr(x), _ptr(u_packed), _ptr(scale), _ptr(bias), _ptr(y), n, h, w, cin, cout, int(relu), _stream()),
           "vatl_deconv4x4s2_winograd_fwd")
    return y


def maxpool3x3s2_fwd(x):
    n, h, w, c = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), device=x.device, dtype=torch.float32)
    _check(lib().vatl_maxpool3x3s2_fwd(_ptr(x), _ptr(y), n, h, w, c, _stream()), "vatl_maxpool3x3s2_fwd")
    return y


def gap_fwd(x):
    n, h, w, c = x.shape
    y = torch.empty((n, c), device=x.device, dtype=torch.float32)
    _check(lib().vatl_gap_fwd(_ptr(x), _ptr(y), n, h * w, c, _stream()), "vatl_gap_fwd")
    return y


def pixelshuffle2_fwd(x):
    n, h, w, c = x.shape
    y = torch.empty((n, 2 * h, 2 * w, c // 4), device=x.device, dtype=torch.float32)
    _check(lib().vatl_pixelshuffle2_fwd(_ptr(x), _ptr(y), n, h, w, c, _stream()), "vatl_pixelshuffle2_fwd")
    return y


def se_scale_add_relu(x, gate, residual):
    n, h, w, c = x.shape
    y = torch.empty_like(x)
    _check(lib().vatl_se_scale_add_relu(_ptr(x), _ptr(gate), _ptr(residual), _ptr(y), n, h * w, c, _stream()), "vatl_se_scale_add_relu")
    return y


def fuse_upsample_add(base, ups, relu: bool):
    """base (N,H,W,C); ups = [(z, shift)] with z (N,H>>shift,W>>shift,C), at most 3."""
    n, h, w, c = base.shape
    y = torch.empty_like(base)
    a = list(ups) + [(None, 0)] * (3 - len(ups))
    _check(lib().vatl_fuse_upsample_add(_ptr(base), _ptr(a[0][0]), a[0][1], _ptr(a[1][0]), a[1][1], _ptr(a[2][0]), a[2][1], _ptr(y),
                                        n, h, w, c, int(relu), _stream()), "vatl_fuse_upsample_add")
    return y


# ----------------------------------------------------------------------------
# flip testing: mirrored crops, and the merge of the mirrored pass's heat-maps (csrc/flip.hip)
# ----------------------------------------------------------------------------

def flip_nchw(x: torch.Tensor, out=None) -> torch.Tensor:
    """The mirror image of fp32 crops (..., W): out[..., w] = x[..., W-1-w], the reference's ``flip`` (transforms.py:479-483).  Out of place."""
    if x.dim() < 1 or x.shape[-1] < 1:
        raise VatlError(f"flip_nchw: no last axis to mirror in shape {tuple(x.shape)}")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    elif out.shape != x.shape or out.device != x.device:
        raise VatlError(f"flip_nchw: out {tuple(out.shape)} on {out.device} does not match x {tuple(x.shape)} on {x.device}")
    w = x.shape[-1]
    _check(lib().vatl_flip_nchw(_ptr(x), _ptr(out), x.numel() // w, w, _stream()), "vatl_flip_nchw")
    return out


def flip_src_joints(joint_pairs, j: int):
    """The joint each output joint takes from the mirrored maps: the swaps of ``joint_pairs`` composed in list order, as the reference's
    flip_heatmap applies them one after another to the current contents (a table that repeats joints gives a general permutation)."""
    src = list(range(j))
    for pair in joint_pairs:
        a, b = (int(v) for v in pair)
        if not (0 <= a < j and 0 <= b < j):
            raise VatlError(f"flip_merge: joint pair ({a}, {b}) is outside [0, {j})")
        src[a], src[b] = src[b], src[a]
    return src


_flip_tables = {}                                    # (pairs, J, device) -> int32 device table of flip_src_joints


def _flip_table(joint_pairs, j: int, device):
    key = (tuple((int(a), int(b)) for a, b in joint_pairs), j, device)
    t = _flip_tables.get(key)
    if t is None:
        t = _flip_tables[key] = upload(torch.tensor(flip_src_joints(key[0], j), dtype=torch.int32), device)
    return t


def flip_merge(hm: torch.Tensor, hm_flip: torch.Tensor, joint_pairs, shift: bool = True) -> torch.Tensor:
    """In place on hm (N,J,H,W): hm = (hm + flip_heatmap(hm_flip, joint_pairs, shift)) / 2 with the reference's bits (transforms.py:486-518,
    :550-552); hm_flip, the heat-maps of the mirrored crops, is only read and must not overlap hm."""
    if hm.dim() != 4 or hm_flip.shape != hm.shape or hm_flip.device != hm.device:
        raise VatlError(f"flip_merge: hm {tuple(hm.shape)} on {hm.device} and hm_flip {tuple(hm_flip.shape)} on {hm_flip.device} must be equal (N,J,H,W) tensors")
    n, j, h, w = hm.shape
    if min(j, h, w) < 1:
        raise VatlError(f"flip_merge: empty heat-maps {tuple(hm.shape)}")
    a, b = _ptr(hm), _ptr(hm_flip)
    _check(lib().vatl_flip_merge(a, b, _ptr(_flip_table(joint_pairs, j, hm.device), torch.int32), n, j, h, w, int(bool(shift)), _stream()), "vatl_flip_merge")
    return hm


# ----------------------------------------------------------------------------
# scorers on (N,J,H,W) heat-maps and decoded poses
# ----------------------------------------------------------------------------

def decode(hm: torch.Tensor, bbox: torch.Tensor):
    """-> coords (N,J,2) f32, maxvals (N,J) f32, idx (N,J) i32."""
    n, j, h, w = hm.shape
    coords = torch.empty((n, j, 2), device=hm.device, dtype=torch.float32)
    maxv = torch.empty((n, j), device=hm.device, dtype=torch.float32)
    idx = torch.empty((n, j), device=hm.device, dtype=torch.int32)
    _check(lib().vatl_decode_argmax_affine(_ptr(hm), _ptr(bbox), _ptr(coords), _ptr(maxv), _ptr(idx, torch.int32), n, j, h, w, _stream()),
           "vatl_decode_argmax_affine")
    return coords, maxv, idx


def decode_pose(hm: torch.Tensor, bbox: torch.Tensor):
    """-> kpts (N,J,3) f32 rows (x, y, score), idx (N,J) i32, hp (N) = -sum of scores, pose_score (N) f64 = float32 mean + 1.25 max in float64 (numpy 1.23 promotion): the decode and the
    per-item scores of ActiveLearning.py:304-314, 329-330 in two launches (no cat / neg / sum / max / mean kernels around them)."""
    n, j, h, w = hm.shape
    kpts = torch.empty((n, j, 3), device=hm.device, dtype=torch.float32)
    idx = torch.empty((n, j), device=hm.device, dtype=torch.int32)
    hp = torch.empty((n,), device=hm.device, dtype=torch.float32)
    ps = torch.empty((n,), device=hm.device, dtype=torch.float64)
    _check(lib().vatl_decode_pose(_ptr(hm), _ptr(bbox), _ptr(kpts), _ptr(idx, torch.int32), _ptr(hp), _ptr(ps, torch.float64), n, j, h, w, _stream()), "vatl_decode_pose")
    return kpts, idx, hp, ps


def decode_softargmax(hm: torch.Tensor, bbox: torch.Tensor, norm_type: str = "softmax"):
    n, j, h, w = hm.shape
    coords = torch.empty((n, j, 2), device=hm.device, dtype=torch.float32)
    scores = torch.empty((n, j), device=hm.device, dtype=torch.float32)
    code = {"softmax": 0, "sigmoid": 1, "divide_sum": 2}.get(norm_type)
    if code is None:
        raise NotImplementedError(norm_type)
    _check(lib().vatl_decode_softargmax(_ptr(hm), _ptr(bbox), _ptr(coords), _ptr(scores), n, j, h, w, code, _stream()), "vatl_decode_softargmax")
    return coords, scores


def peaks5(hm: torch.Tensor, min_distance: int = 5):
    """(N,J,H,W) -> peak values (N,J,5), flat indices (N,J,5) int32 (-1 = none), counts (N,J) int32, MPE terms (N,J),
    Margin terms (N,J)   [skimage.feature.peak_local_max(min_distance, num_peaks=5) per plane]."""
    n, j, h, w = hm.shape
    val = torch.empty((n, j, 5), device=hm.device, dtype=torch.float32)
    idx = torch.empty((n, j, 5), device=hm.device, dtype=torch.int32)
    cnt = torch.empty((n, j), device=hm.device, dtype=torch.int32)
    mpe = torch.empty((n, j), device=hm.device, dtype=torch.float32)
    mar = torch.empty((n, j), device=hm.device, dtype=torch.float32)
    _check(lib().vatl_peaks5(_ptr(hm), _ptr(val), _ptr(idx, torch.int32), _ptr(cnt, torch.int32), _ptr(mpe), _ptr(mar), n, j, h, w, min_distance,
                             _stream()), "vatl_peaks5")
    return val, idx, cnt, mpe, mar


def plane_entropy(hm: torch.Tensor) -> torch.Tensor:
    n, j, h, w = hm.shape
    out = torch.empty((n, j), device=hm.device, dtype=torch.float32)
    _check(lib().vatl_plane_entropy(_ptr(hm), _ptr(out), n, j, h, w, _stream()), "vatl_plane_entropy")
    return out


def localpeak_mean(hm: torch.Tensor, order: float = 0.5):
    """-> mean (N,) f32 (nan when no peak is kept), count (N,J) i32."""
    n, j, h, w = hm.shape
    mean = torch.empty(n, device=hm.device, dtype=torch.float32)
    cnt = torch.empty((n, j), device=hm.device, dtype=torch.int32)
    ws = torch.empty(2 * n * j, device=hm.device, dtype=torch.float64)
    _check(lib().vatl_localpeak_mean(_ptr(hm), _ptr(mean), _ptr(cnt, torch.int32), _ptr(ws, torch.float64), n, j, h, w, order, _stream()),
           "vatl_localpeak_mean")
    return mean, cnt


def localpeak_mask(hm: torch.Tensor, order: float = 0.5) -> torch.Tensor:
    """hm (..., H, W) -> uint8 mask of kept local peaks, same shape."""
    h, w = hm.shape[-2:]
    planes = hm.numel() // (h * w)
    mask = torch.empty(hm.shape, device=hm.device, dtype=torch.uint8)
    _check(lib().vatl_localpeak_mask(_ptr(hm), _ptr(mask, torch.uint8), planes, h, w, order, _stream()), "vatl_localpeak_mask")
    return mask


def thc_pairs(a: torch.Tensor, b: torch.Tensor, norm: str = "L1") -> torch.Tensor:
    """a, b (P,J,H,W) (views with a uniform item stride are fine) -> (P,) f32."""
    p, j, h, w = a.shape
    for t in (a, b):
        if not t.is_cuda or t.dtype != torch.float32 or t[0].is_contiguous() is False:
            raise VatlError("thc_pairs: fp32 device tensors with contiguous items required")
    out = torch.empty(p, device=a.device, dtype=torch.float32)
    sa = a.stride(0) if p > 1 else j * h * w
    sb = b.stride(0) if p > 1 else j * h * w
    _check(lib().vatl_thc_pairs(a.data_ptr(), b.data_ptr(), sa, sb, _ptr(out), p, j, h * w, {"L1": 1, "L2": 2}[norm], _stream()), "vatl_thc_pairs")
    return out


def thc_stream(hm: torch.Tensor, is_prev: torch.Tensor, is_next: torch.Tensor, norm: str = "L1") -> torch.Tensor:
    """THC of an id-sorted, de-duplicated stream: neighbours are items i-1 / i+1."""
    n = hm.shape[0]
    thc = torch.empty(n, device=hm.device, dtype=torch.float32)
    pair = thc_pairs(hm[:-1], hm[1:], norm) if n > 1 else None
    _check(lib().vatl_thc_combine(_ptr(pair), _ptr(is_prev, torch.uint8), _ptr(is_next, torch.uint8), _ptr(thc), n, _stream()), "vatl_thc_combine")
    return thc


def tpc_stream(hm: torch.Tensor, bbox: torch.Tensor, cur_coords: torch.Tensor, is_prev: torch.Tensor, is_next: torch.Tensor) -> torch.Tensor:
    """TPC of an id-sorted de-duplicated stream (neighbours = items i-1 / i+1, decoded with item i's box)."""
    n, j = hm.shape[:2]
    adj_prev = torch.zeros((n, j, 2), device=hm.device, dtype=torch.float32)
    adj_next = torch.zeros((n, j, 2), device=hm.device, dtype=torch.float32)
    if n > 1:
        h, w = hm.shape[2:]
        scratch = torch.empty((n - 1, j), device=hm.device, dtype=torch.float32)
        _check(lib().vatl_decode_argmax_affine(hm[:-1].data_ptr(), bbox[1:].data_ptr(), adj_prev[1:].data_ptr(), _ptr(scratch), None,
                                               n - 1, j, h, w, _stream()), "vatl_decode_argmax_affine")
        _check(lib().vatl_decode_argmax_affine(hm[1:].data_ptr(), bbox[:-1].data_ptr(), adj_next[:-1].data_ptr(), _ptr(scratch), None,
                                               n - 1, j, h, w, _stream()), "vatl_decode_argmax_affine")
    out = torch.empty(n, device=hm.device, dtype=torch.float32)
    _check(lib().vatl_tpc_stream(_ptr(cur_coords), _ptr(adj_prev), _ptr(adj_next), _ptr(bbox), _ptr(is_prev, torch.uint8),
                                 _ptr(is_next, torch.uint8), _ptr(out), n, j, _stream()), "vatl_tpc_stream")
    return out


def pack_ae(state_dict, device) -> torch.Tensor:
    parts = []
    for half in ("encoder", "decoder"):
        for i in (0, 2, 4, 6):
            parts.append(state_dict[f"{half}.{i}.weight"].detach().reshape(-1).float())
            parts.append(state_dict[f"{half}.{i}.bias"].detach().reshape(-1).float())
    return torch.cat([p.to(device) for p in parts]).contiguous()


def ae_forward(feat: torch.Tensor, ae_flat: torch.Tensor, d: int, z: int, want_recon: bool = True):
    """feat (N,D) -> recon (N,D) (None without ``want_recon``), mse (N,)."""
    n = feat.shape[0]
    recon = torch.empty((n, d), device=feat.device, dtype=torch.float32) if want_recon else None
    mse = torch.empty(n, device=feat.device, dtype=torch.float32)
    _check(lib().vatl_ae_forward(_ptr(feat), _ptr(ae_flat), d, z, _ptr(recon), _ptr(mse), n, _stream()), "vatl_ae_forward")
    return recon, mse


def hybrid_ae_wpu(kpts: torch.Tensor, bbox: torch.Tensor, ae_flat: torch.Tensor, d: int, z: int, only38: bool = False):
    """kpts (N,17,3), bbox (N,4) crop xyxy -> wpu (N,) f32, status (N,) i32."""
    n = kpts.shape[0]
    wpu = torch.empty(n, device=kpts.device, dtype=torch.float32)
    status = torch.empty(n, device=kpts.device, dtype=torch.int32)
    _check(lib().vatl_hybrid_ae_wpu(_ptr(kpts), _ptr(bbox), _ptr(ae_flat), d, z, int(only38), _ptr(wpu), _ptr(status, torch.int32), n, _stream()),
           "vatl_hybrid_ae_wpu")
    return wpu, status


def hybrid_feature_f64(kpts: torch.Tensor, bbox_xywh: torch.Tensor):
    """kpts (N,51) f64, bbox (N,4) f64 xywh -> feat (N,42) f64, status (N,) i32."""
    n = kpts.shape[0]
    feat = torch.empty((n, 42), device=kpts.device, dtype=torch.float64)
    status = torch.empty(n, device=kpts.device, dtype=torch.int32)
    _check(lib().vatl_hybrid_feature_f64(_ptr(kpts, torch.float64), _ptr(bbox_xywh, torch.float64), _ptr(feat, torch.float64),
                                         _ptr(status, torch.int32), n, _stream()), "vatl_hybrid_feature_f64")
    return feat, status


# ----------------------------------------------------------------------------
# evaluation and query selection
# ----------------------------------------------------------------------------

def oks(pred_kpts: torch.Tensor, gt_kpts: torch.Tensor, bbox_xywh: torch.Tensor) -> torch.Tensor:
    """pred (N,17,3) fp32, gt (N,51) float64, boxes (N,4) xywh float64 -> (N,) float64 OKS."""
    n = pred_kpts.shape[0]
    out = torch.empty(n, device=pred_kpts.device, dtype=torch.float64)
    _check(lib().vatl_oks(_ptr(pred_kpts), _ptr(gt_kpts, torch.float64), _ptr(bbox_xywh, torch.float64), _ptr(out, torch.float64), n, _stream()),
           "vatl_oks")
    return out


def _query_emb(emb):
    if emb.dim() != 2 or emb.dtype != torch.float32 or not emb.is_contiguous():
        raise ValueError(f"embeddings must be a contiguous 2-D float32 tensor, got {tuple(emb.shape)} {emb.dtype}")
    return emb.shape


def _query_vec(t, name, need, dtype=torch.float64):
    """Host-side length / type check of a vector the query kernels index up to ``need`` entries of (shapes only: no device read)."""
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < need:
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of at least {need} entries, got {t.numel()} of {t.dtype}")


def cosine_rowsum(emb: torch.Tensor) -> torch.Tensor:
    """(n, D) fp32 -> (n,) float64 sums of cosine distances to every row (incl. itself: 0; a zero row: n - 1)."""
    n, d = _query_emb(emb)
    out = torch.empty(n, device=emb.device, dtype=torch.float64)
    ws = torch.empty(n + d, device=emb.device, dtype=torch.float64)
    _check(lib().vatl_cosine_rowsum(_ptr(emb), n, d, _ptr(out, torch.float64), _ptr(ws, torch.float64), _stream()), "vatl_cosine_rowsum")
    return out


def kcenter_update(emb, centers: torch.Tensor, min_dist: torch.Tensor, first: bool):
    """min_dist[:n] = min(min_dist[:n], distance to the nearest of ``centers``) (``first``: no previous value).  ``centers`` holds
    row indices below n on the device; they are the caller's to keep in range (they are not read back here)."""
    n, _ = _query_emb(emb)
    _query_vec(centers, "centers", 0, torch.int32)
    _query_vec(min_dist, "min_dist", n)
    _check(lib().vatl_kcenter_update(_ptr(emb), emb.shape[0], emb.shape[1], _ptr(centers, torch.int32), centers.numel(), _ptr(min_dist, torch.float64),
                                     int(first), _stream()), "vatl_kcenter_update")


def kcenter_pick(min_dist, unc, a: float, b: float, selected: torch.Tensor, step: int, n: int):
    """selected[step] = np.argmax(a * min_dist[:n] + b * unc[:n]) (a missing array counts as zeros); then unc[selected[step]] = 0."""
    if n <= 0 or step < 0 or (min_dist is None and unc is None):
        raise ValueError(f"kcenter_pick: need n > 0, step >= 0 and at least one score array (n={n}, step={step})")
    if min_dist is not None:
        _query_vec(min_dist, "min_dist", n)
    if unc is not None:
        _query_vec(unc, "unc", n)
    _query_vec(selected, "selected", step + 1, torch.int32)
    _check(lib().vatl_kcenter_pick(_ptr(min_dist, torch.float64), _ptr(unc, torch.float64), a, b, _ptr(selected, torch.int32), step, n, _stream()),
           "vatl_kcenter_pick")


def _f64(t):
    return _ptr(t, torch.float64)


def _i32(t):
    return _ptr(t, torch.int32)


def kmeans_prepare(emb: torch.Tensor):
    """(n, D) fp32 -> centred float64 copy (n, D), column means (D), tol (1): mean(var(X, axis=0)) * 1e-4."""
    n, d = emb.shape
    xc = torch.empty((n, d), device=emb.device, dtype=torch.float64)
    mean = torch.empty(d, device=emb.device, dtype=torch.float64)
    tol = torch.empty(1, device=emb.device, dtype=torch.float64)
    ws = torch.empty(max(d, 1), device=emb.device, dtype=torch.float64)
    _check(lib().vatl_kmeans_prepare(_ptr(emb), n, d, _f64(xc), _f64(mean), _f64(tol), _f64(ws), _stream()), "vatl_kmeans_prepare")
    return xc, mean, tol


def kmeans_seed(xc: torch.Tensor, weight: torch.Tensor, k: int, first_index: int, draws: torch.Tensor, trials: int) -> torch.Tensor:
    """k-means++ on the centred rows with the host's random draws ((k-1) * trials doubles on the device).  Returns int32 (k + 1):
    the k seeding indices, then the tie flag."""
    n, d = xc.shape
    out = torch.zeros(k + 1, device=xc.device, dtype=torch.int32)
    ws = torch.empty(max(int(lib().vatl_kmeans_seed_workspace_doubles(n, trials)), 1), device=xc.device, dtype=torch.float64)
    _check(lib().vatl_kmeans_seed(_f64(xc), _f64(weight), n, d, k, first_index, _f64(draws), trials, _i32(out), out.data_ptr() + 4 * k, _f64(ws),
                                  _stream()), "vatl_kmeans_seed")
    return out


def kmeans_assign(xc, centers, labels_prev, labels, status, workspace):
    """labels <- nearest centre (f64 MFMA); status[0] <- 1.0 when a label differs from labels_prev (None: always)."""
    _check(lib().vatl_kmeans_assign(_f64(xc), _f64(centers), xc.shape[0], xc.shape[1], centers.shape[0], _i32(labels_prev), _i32(labels), _f64(status),
                                    _f64(workspace), _stream()), "vatl_kmeans_assign")


def kmeans_update_workspace_doubles(d: int, k: int) -> int:
    return int(lib().vatl_kmeans_update_workspace_doubles(d, k))


def kmeans_update(xc, weight, labels, centers, centers_new, status, workspace):
    """centers_new <- weighted cluster means; status[1] <- total squared shift, status[2] <- 1.0 when a cluster has no weight."""
    _check(lib().vatl_kmeans_update(_f64(xc), _f64(weight), _i32(labels), _f64(centers), xc.shape[0], xc.shape[1], centers.shape[0], _f64(centers_new),
                                    _f64(status), _f64(workspace), _stream()), "vatl_kmeans_update")


def kmeans_finish(emb, xc, mean, weight, centers, labels) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (representatives int32 (k): per cluster the member nearest its centre, -1 without members; inertia float64 (1))."""
    n, d = xc.shape
    k = centers.shape[0]
    reps = torch.empty(k, device=xc.device, dtype=torch.int32)
    inertia = torch.empty(1, device=xc.device, dtype=torch.float64)
    ws = torch.empty(2 * n, device=xc.device, dtype=torch.float64)
    _check(lib().vatl_kmeans_finish(_ptr(emb), _f64(xc), _f64(mean), _f64(weight), _f64(centers), _i32(labels), n, d, k, _i32(reps), _f64(inertia),
                                    _f64(ws), _stream()), "vatl_kmeans_finish")
    return reps, inertia


# ----------------------------------------------------------------------------
# training-mode backbone ops (NHWC): forward
# ----------------------------------------------------------------------------

def conv2d_fwd_ex(x, w_packed, cout, r, s, stride, pad_y, pad_x, ho, wo, oh, ow, osy, osx, ooy, oox, out=None, residual=None,
                  scale=None, bias=None, relu=False):
    n, h, w, cin = x.shape
    y = out if out is not None else torch.empty((n, oh, ow, cout), device=x.device, dtype=torch.float32)
    _check(lib().vatl_conv2d_fwd_ex(_ptr(x), _ptr(w_packed), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, cin, cout,
                                    w_packed.shape[0], r, s, stride, pad_y, pad_x, ho, wo, oh, ow, osy, osx, ooy, oox, int(relu), _stream()),
           "vatl_conv2d_fwd_ex")
    return y


def scale_bias_act(z, scale, bias, residual=None, relu=True):
    c = z.shape[-1]
    y = torch.empty_like(z)
    _check(lib().vatl_scale_bias_act(_ptr(z), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(y), z.numel() // c, c, int(relu), _stream()),
           "vatl_scale_bias_act")
    return y


def _col_ws(m: int, c: int, device):
    return torch.empty(int(lib().vatl_col_reduce_workspace_doubles(m, c)), device=device, dtype=torch.float64)


def bn_train_fwd_stats(z, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """z NHWC (..., C) -> save_mean, save_invstd, scale, bias (C,); running stats updated in place."""
    c = z.shape[-1]
    m = z.numel() // c
    outs = [torch.empty(c, device=z.device, dtype=torch.float32) for _ in range(4)]
    _check(lib().vatl_bn_train_fwd_stats(_ptr(z), m, c, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), momentum, eps,
                                         _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(_col_ws(m, c, z.device), torch.float64),
                                         _stream()), "vatl_bn_train_fwd_stats")
    return outs


def _bn_finalize(stats, nblk, m, c, bn_args, device):
    gamma, beta, running_mean, running_var, momentum, eps = bn_args
    outs = [torch.empty(c, device=device, dtype=torch.float32) for _ in range(4)]
    _check(lib().vatl_bn_train_finalize(_ptr(stats, torch.float64), nblk, m, c, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                        momentum, eps, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _stream()), "vatl_bn_train_finalize")
    return outs


def _stats_fwd(fn: str, x, w_packed, z_shape, row_blocks: int, dims, bn_args=None):
    """The training forwards that take the statistics of z in the conv epilogue: allocate z and the float64 (sum, sum^2) partials of
    the ``row_blocks`` row blocks the launch may write, run ``fn(x, w, z, partials, &used, *dims, stream)``.  -> z, partials, row
    blocks written; with ``bn_args`` = (gamma, beta, running_mean, running_var, momentum, eps) the partials are finalized instead:
    -> [z, save_mean, save_invstd, scale, bias], running stats updated in place."""
    cout = z_shape[-1]
    z = torch.empty(z_shape, device=x.device, dtype=torch.float32)
    stats = torch.empty(int(row_blocks) * cout * 2, device=x.device, dtype=torch.float64)
    used = C.c_int64(0)
    _check(getattr(lib(), fn)(_ptr(x), _ptr(w_packed), _ptr(z), _ptr(stats, torch.float64), C.addressof(used), *dims, _stream()), fn)
    if bn_args is None:
        return z, stats, used.value
    return [z] + _bn_finalize(stats, used.value, z.numel() // cout, cout, bn_args, x.device)


def conv2d_fwd_bnstats(x, w_packed, cout: int, r: int, s: int, stride: int, pad: int, gamma, beta, running_mean, running_var,
                       momentum: float, eps: float):
    """Training forward: z = conv(x) with the BatchNorm batch statistics taken in the conv epilogue.
    -> z, save_mean, save_invstd, scale, bias; running stats updated in place."""
    n, h, w, cin = x.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    return _stats_fwd("vatl_conv2d_fwd_stats", x, w_packed, (n, ho, wo, cout), lib().vatl_conv_stats_row_blocks(n * ho * wo, 1),
                      (n, h, w, cin, cout, w_packed.shape[0], r, s, stride, pad), (gamma, beta, running_mean, running_var, momentum, eps))


def deconv4x4s2_fwd_bnstats(x, w_packed, cout: int, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    n, h, w, cin = x.shape
    return _stats_fwd("vatl_deconv4x4s2_fwd_stats", x, w_packed, (n, 2 * h, 2 * w, cout), lib().vatl_conv_stats_row_blocks(n * h * w, 4),
                      (n, h, w, cin, cout, w_packed.shape[1]), (gamma, beta, running_mean, running_var, momentum, eps))


def conv3x3_winograd_fwd_stats(x, u_packed, cout: int):
    """Training forward of a 3x3 / stride-1 layer through Winograd: z = conv(x) and the row-block (sum, sum^2) partials of z.
    -> z, stats (float64), row blocks written."""
    n, h, w, cin = x.shape
    return _stats_fwd("vatl_conv3x3_winograd_fwd_stats", x, u_packed, (n, h, w, cout), lib().vatl_winograd_stats_row_blocks(n, h, w), (n, h, w, cin, cout))


def conv3x3_winograd_fwd_bnstats(x, u_packed, cout: int, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """conv2d_fwd_bnstats for the Winograd route: -> z, save_mean, save_invstd, scale, bias; running stats updated in place."""
    z, stats, used = conv3x3_winograd_fwd_stats(x, u_packed, cout)
    return [z] + _bn_finalize(stats, used, z.numel() // cout, cout, (gamma, beta, running_mean, running_var, momentum, eps), x.device)


def conv3x3_winograd_f4_fwd_bnstats(x, u, cout: int, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """conv3x3_winograd_fwd_bnstats on the F(4x4,3x3) route: -> z, save_mean, save_invstd, scale, bias; running stats updated in place."""
    n, h, w, cin = x.shape
    return _stats_fwd("vatl_conv3x3_winograd_f4_fwd_stats", x, u, (n, h, w, cout), lib().vatl_winograd_f4_stats_row_blocks(n, h, w), (n, h, w, cin, cout),
                      (gamma, beta, running_mean, running_var, momentum, eps))


def deconv4x4s2_winograd_fwd_bnstats(x, u_packed, cout: int, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """deconv4x4s2_fwd_bnstats on the Winograd route: -> z, save_mean, save_invstd, scale, bias; running stats updated in place."""
    n, h, w, cin = x.shape
    return _stats_fwd("vatl_deconv4x4s2_winograd_fwd_stats", x, u_packed, (n, 2 * h, 2 * w, cout), lib().vatl_winograd_deconv_stats_row_blocks(n, h, w),
                      (n, h, w, cin, cout), (gamma, beta, running_mean, running_var, momentum, eps))


def maxpool3x3s2_fwd_idx(x):
    n, h, w, c = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), device=x.device, dtype=torch.float32)
    idx = torch.empty(y.shape, device=x.device, dtype=torch.uint8)
    _check(lib().vatl_maxpool3x3s2_fwd_idx(_ptr(x), _ptr(y), _ptr(idx, torch.uint8), n, h, w, c, _stream()), "vatl_maxpool3x3s2_fwd_idx")
    return y, idx


def maxpool3x3s2_fwd_idx_affine(z, scale, bias):
    """pool(relu(z*scale + bias)) and the winning taps in one pass over the conv output z (the activation is never stored)."""
    n, h, w, c = z.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), device=z.device, dtype=torch.float32)
    idx = torch.empty(y.shape, device=z.device, dtype=torch.uint8)
    _check(lib().vatl_maxpool3x3s2_fwd_idx_affine(_ptr(z), _ptr(scale), _ptr(bias), _ptr(y), _ptr(idx, torch.uint8), n, h, w, c, _stream()),
           "vatl_maxpool3x3s2_fwd_idx_affine")
    return y, idx


# ----------------------------------------------------------------------------
# training-mode backbone ops: data gradients with the BatchNorm-backward epilogue
# ----------------------------------------------------------------------------

class BnBwdSpec:
    """What a data-gradient launch needs to run the reduction pass of the consumer layer's BatchNorm backward in its
    epilogue: z (the consumer's conv output), its ReLU mask source (mask_y, or (scale, bias) to recompute it from z, or
    neither) and the saved batch statistics.  ``stats`` / ``blocks`` collect the partial sums of one or more launches."""

    def __init__(self, z, mean, invstd, mask_y=None, scale=None, bias=None):
        self.z, self.mean, self.invstd, self.mask_y, self.scale, self.bias = z, mean, invstd, mask_y, scale, bias
        c = z.shape[-1]
        cap = int(lib().vatl_conv_stats_row_blocks(z.numel() // c, 1)) + 8     # + a partial tile per parity launch
        self.stats = torch.empty(cap * c * 2, device=z.device, dtype=torch.float64)
        self.blocks = 0

    def window(self, need: int, who: str) -> int:
        """Address of the free tail of ``stats`` for a launch of ``who`` that may write ``need`` more row blocks (2 doubles per
        channel each) — raises when they do not fit: this is the only guard in front of that launch's device writes."""
        c = self.z.shape[-1]
        if (self.blocks + need) * c * 2 > self.stats.numel():
            raise VatlError(f"{who}: statistics buffer too small")
        return self.stats.data_ptr() + self.blocks * c * 2 * 8

    def advance(self, used: C.c_int64):
        """The launch that was given ``window()`` wrote this many row blocks."""
        self.blocks += used.value


def _bnbwd_tail(spec: BnBwdSpec, y, need: int, who: str):
    """-> (used, the eight trailing arguments of a *_bnbwd entry point before the stream: z, mask_y, scale, bias, mean, invstd, the
    statistics window, &used) for a launch of ``who`` that writes ``y`` and at most ``need`` row blocks of partials."""
    if y.shape != spec.z.shape:
        raise VatlError(f"{who}: the BatchNorm tensors must have the layout of the output")
    used = C.c_int64(0)
    return used, (_ptr(spec.z), _ptr(spec.mask_y), _ptr(spec.scale), _ptr(spec.bias), _ptr(spec.mean), _ptr(spec.invstd),
                  spec.window(need, who), C.addressof(used))


def conv2d_fwd_ex_bnbwd(x, w_packed, cout, r, s, stride, pad_y, pad_x, ho, wo, oh, ow, osy, osx, ooy, oox, spec: BnBwdSpec, out=None, residual=None):
    """conv2d_fwd_ex whose epilogue masks the result with the consumer layer's ReLU and appends the (sum g, sum g*xhat) row-block
    partials to ``spec`` (several launches — the parity launches of a strided conv's data gradient — append one after another)."""
    n, h, w, cin = x.shape
    y = out if out is not None else torch.empty((n, oh, ow, cout), device=x.device, dtype=torch.float32)
    used, tail = _bnbwd_tail(spec, y, int(lib().vatl_conv_stats_row_blocks(n * ho * wo, 1)), "conv2d_fwd_ex_bnbwd")
    _check(lib().vatl_conv2d_fwd_ex_bnbwd(_ptr(x), _ptr(w_packed), _ptr(residual), _ptr(y), n, h, w, cin, cout, w_packed.shape[0], r, s, stride, pad_y,
                                          pad_x, ho, wo, oh, ow, osy, osx, ooy, oox, *tail, _stream()), "vatl_conv2d_fwd_ex_bnbwd")
    spec.advance(used)
    return y


def conv3x3_winograd_fwd_bnbwd(x, u_packed, cout: int, spec: "BnBwdSpec", out=None, residual=None):
    """conv2d_fwd_ex_bnbwd for the 3x3 / stride-1 data gradients on the Winograd route (u_packed: data-gradient packing)."""
    n, h, w, cin = x.shape
    y = out if out is not None else torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    used, tail = _bnbwd_tail(spec, y, int(lib().vatl_winograd_stats_row_blocks(n, h, w)), "conv3x3_winograd_fwd_bnbwd")
    _check(lib().vatl_conv3x3_winograd_fwd_bnbwd(_ptr(x), _ptr(u_packed), _ptr(residual), _ptr(y), n, h, w, cin, cout, *tail, _stream()),
           "vatl_conv3x3_winograd_fwd_bnbwd")
    spec.advance(used)
    return y


def conv3x3_winograd_f4_fwd_bnbwd(x, u, cout: int, spec: "BnBwdSpec", out=None, residual=None):
    """conv3x3_winograd_fwd_bnbwd on the F(4x4,3x3) route (u: data-gradient packing)."""
    n, h, w, cin = x.shape
    y = out if out is not None else torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    used, tail = _bnbwd_tail(spec, y, int(lib().vatl_winograd_f4_stats_row_blocks(n, h, w)), "conv3x3_winograd_f4_fwd_bnbwd")
    _check(lib().vatl_conv3x3_winograd_f4_fwd_bnbwd(_ptr(x), _ptr(u), _ptr(residual), _ptr(y), n, h, w, cin, cout, *tail, _stream()),
           "vatl_conv3x3_winograd_f4_fwd_bnbwd")
    spec.advance(used)
    return y


def deconv4x4s2_winograd_dgrad(dz, u_packed, cin: int, spec: "BnBwdSpec" = None, residual=None, out=None):
    """dx (N,H,W,Cin) of ConvTranspose2d(4,2,1) from dz (N,2H,2W,Cout); with ``spec`` the epilogue masks the result with the consumer
    layer's ReLU and appends the (sum g, sum g*xhat) row-block partials (conv2d_fwd_ex_bnbwd semantics)."""
    n, h2, w2, cout = dz.shape
    h, w = h2 // 2, w2 // 2
    dx = out if out is not None else torch.empty((n, h, w, cin), device=dz.device, dtype=torch.float32)
    if spec is None:
        _check(lib().vatl_deconv4x4s2_winograd_dgrad(_ptr(dz), _ptr(u_packed), _ptr(residual), _ptr(dx), n, h, w, cin, cout, _stream()),
               "vatl_deconv4x4s2_winograd_dgrad")
        return dx
    # one grid of F(3x3,2x2) tiles over (N,H,W): the transposed conv's forward statistics count four phases of exactly this grid
    used, tail = _bnbwd_tail(spec, dx, int(lib().vatl_winograd_deconv_stats_row_blocks(n, h, w)) // 4, "deconv4x4s2_winograd_dgrad")
    _check(lib().vatl_deconv4x4s2_winograd_dgrad_bnbwd(_ptr(dz), _ptr(u_packed), _ptr(residual), _ptr(dx), n, h, w, cin, cout, *tail, _stream()),
           "vatl_deconv4x4s2_winograd_dgrad_bnbwd")
    spec.advance(used)
    return dx


# ----------------------------------------------------------------------------
# training-mode backbone ops: weight gradients
# ----------------------------------------------------------------------------

def _grad_out(who: str, out, shape, ws_floats: int, device):
    """-> (dw, workspace) of a weight-gradient launch: ``out`` (a slice of the flat gradient arena; any shape with the right element
    count) or a fresh tensor of ``shape``, and the launch's float workspace."""
    dw = out if out is not None else torch.empty(shape, device=device, dtype=torch.float32)
    if dw.numel() != shape[0] * shape[1] * shape[2] * shape[3]:
        raise VatlError(f"{who}: out has the wrong size")
    return dw, torch.empty(int(ws_floats), device=device, dtype=torch.float32)


def _check_grad_pair(who: str, x, g, cx: int, grid):
    """The two operands of a weight-gradient launch describe the same batch: x (N,H,W,cx) and the gradient (N,*grid,C).  The kernels
    take the pixel grid from x and the filter geometry alone; a gradient of another grid would be read with the wrong strides."""
    if x.dim() != 4 or g.dim() != 4:
        raise VatlError(f"{who}: operands must be NHWC (4-D), got {tuple(x.shape)} and {tuple(g.shape)}")
    if x.shape[3] != cx:
        raise VatlError(f"{who}: input has {x.shape[3]} channels, the layer reads {cx}")
    if min(grid) < 1 or (g.shape[0], g.shape[1], g.shape[2]) != (x.shape[0], *grid):
        raise VatlError(f"{who}: gradient {tuple(g.shape)} does not match the batch {x.shape[0]} and the grid {grid[0]}x{grid[1]} that the "
                        f"input {tuple(x.shape)} gives")


def conv2d_wgrad(x, dz, cout: int, cin: int, r: int, s: int, stride: int, pad: int, out=None) -> torch.Tensor:
    """x NHWC (N,H,W,Cin or 4 for the stem), dz NHWC (N,Ho,Wo,CoutG) -> dw (Cout,Cin,R,S) (written into ``out`` when
    given: a slice of the flat gradient arena)."""
    _check_grad_pair("conv2d_wgrad", x, dz, 4 if cin == 3 else cin, ((x.shape[1] + 2 * pad - r) // stride + 1, (x.shape[2] + 2 * pad - s) // stride + 1))
    n, h, w, _ = x.shape
    m = n * dz.shape[1] * dz.shape[2]
    dw, ws = _grad_out("conv2d_wgrad", out, (cout, cin, r, s), lib().vatl_conv2d_wgrad_workspace_floats(cout, cin, r, s, m), x.device)
    _check(lib().vatl_conv2d_wgrad(_ptr(x), _ptr(dz), _ptr(dw), _ptr(ws), n, h, w, cin, cout, dz.shape[3], r, s, stride, pad, _stream()),
           "vatl_conv2d_wgrad")
    return dw


def conv3x3_winograd_wgrad(x, dz, out=None) -> torch.Tensor:
    """Weight gradient of a 3x3 / stride 1 / pad 1 conv on the Winograd route: x (N,H,W,Cin), dz (N,H,W,Cout) -> dw (Cout,Cin,3,3)."""
    _check_grad_pair("conv3x3_winograd_wgrad", x, dz, x.shape[-1], tuple(x.shape[1:3]))
    n, h, w, cin = x.shape
    cout = dz.shape[3]
    dw, ws = _grad_out("conv3x3_winograd_wgrad", out, (cout, cin, 3, 3), lib().vatl_conv3x3_winograd_wgrad_workspace_floats(cout, cin, n, h, w), x.device)
    _check(lib().vatl_conv3x3_winograd_wgrad(_ptr(x), _ptr(dz), _ptr(dw), _ptr(ws), n, h, w, cin, cout, _stream()), "vatl_conv3x3_winograd_wgrad")
    return dw


def deconv4x4s2_winograd_wgrad(x, dy, out=None) -> torch.Tensor:
    """Weight gradient of ConvTranspose2d(4,2,1) on the Winograd route: x (N,H,W,Cin), dy (N,2H,2W,Cout) -> dw (Cin,Cout,4,4)."""
    _check_grad_pair("deconv4x4s2_winograd_wgrad", x, dy, x.shape[-1], (2 * x.shape[1], 2 * x.shape[2]))
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    dw, ws = _grad_out("deconv4x4s2_winograd_wgrad", out, (cin, cout, 4, 4), lib().vatl_deconv4x4s2_winograd_wgrad_workspace_floats(cin, cout, n, h, w), x.device)
    _check(lib().vatl_deconv4x4s2_winograd_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), n, h, w, cin, cout, _stream()), "vatl_deconv4x4s2_winograd_wgrad")
    return dw


def deconv4x4s2_wgrad(x, dy, out=None) -> torch.Tensor:
    """Weight gradient of ConvTranspose2d(4,2,1) as an implicit GEMM: x (N,H,W,Cin), dy (N,2H,2W,Cout) -> dw (Cin,Cout,4,4)."""
    _check_grad_pair("deconv4x4s2_wgrad", x, dy, x.shape[-1], (2 * x.shape[1], 2 * x.shape[2]))
    n, h, w, cin = x.shape
    cout = dy.shape[3]
    dw, ws = _grad_out("deconv4x4s2_wgrad", out, (cin, cout, 4, 4), lib().vatl_deconv4x4s2_wgrad_workspace_floats(cin, cout, n * h * w), x.device)
    _check(lib().vatl_deconv4x4s2_wgrad(_ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), n, h, w, cin, cout, _stream()), "vatl_deconv4x4s2_wgrad")
    return dw


# ----------------------------------------------------------------------------
# training-mode backbone ops: BatchNorm and element-wise backward passes
# ----------------------------------------------------------------------------

def _bn_bwd_outs(z, dgamma, dbeta):
    """-> dz, dgamma, dbeta (the given arena slices, or fresh), and the kernels' 3C coefficient scratch."""
    c = z.shape[-1]
    return (torch.empty_like(z), dgamma if dgamma is not None else torch.empty(c, device=z.device, dtype=torch.float32),
            dbeta if dbeta is not None else torch.empty(c, device=z.device, dtype=torch.float32), torch.empty(3 * c, device=z.device, dtype=torch.float32))


def bn_bwd_from_stats(spec: BnBwdSpec, g, gamma, dgamma=None, dbeta=None):
    """Finish the BatchNorm backward whose reduction ran in the data-gradient epilogue: -> dz, dgamma, dbeta."""
    z = spec.z
    c = z.shape[-1]
    m = z.numel() // c
    dz, dgamma, dbeta, coef = _bn_bwd_outs(z, dgamma, dbeta)
    _check(lib().vatl_bn_bwd_from_stats(_ptr(spec.stats, torch.float64), spec.blocks, _ptr(g), _ptr(z), _ptr(gamma), _ptr(spec.mean), _ptr(spec.invstd),
                                        _ptr(dz), _ptr(dgamma), _ptr(dbeta), m, c, _ptr(coef), _stream()), "vatl_bn_bwd_from_stats")
    return dz, dgamma, dbeta


def bn_train_bwd_relu(dy, scale, bias, z, gamma, save_mean, save_invstd, dgamma=None, dbeta=None):
    """Backward of Conv+BN+ReLU without a skip input; the ReLU mask is recomputed from z. -> dz, dgamma, dbeta."""
    c = z.shape[-1]
    m = z.numel() // c
    dz, dgamma, dbeta, coef = _bn_bwd_outs(z, dgamma, dbeta)
    _check(lib().vatl_bn_train_bwd_relu(_ptr(dy), _ptr(scale), _ptr(bias), _ptr(z), _ptr(gamma), _ptr(save_mean), _ptr(save_invstd), _ptr(dz),
                                        _ptr(dgamma), _ptr(dbeta), m, c, _ptr(coef), _ptr(_col_ws(m, c, z.device), torch.float64), _stream()),
           "vatl_bn_train_bwd_relu")
    return dz, dgamma, dbeta


def bn_train_bwd(dy, y, z, gamma, save_mean, save_invstd, want_g: bool = False, dgamma=None, dbeta=None):
    """-> dz, g (or None), dgamma, dbeta."""
    c = z.shape[-1]
    m = z.numel() // c
    dz, dgamma, dbeta, coef = _bn_bwd_outs(z, dgamma, dbeta)
    g = torch.empty_like(z) if want_g else None
    _check(lib().vatl_bn_train_bwd(_ptr(dy), _ptr(y), _ptr(z), _ptr(gamma), _ptr(save_mean), _ptr(save_invstd), _ptr(dz), _ptr(g),
                                   _ptr(dgamma), _ptr(dbeta), m, c, _ptr(coef), _ptr(_col_ws(m, c, z.device), torch.float64), _stream()),
           "vatl_bn_train_bwd")
    return dz, g, dgamma, dbeta


def bn_train_bwd_relu_pool(dpool, idx, scale, bias, z, gamma, save_mean, save_invstd, dgamma=None, dbeta=None):
    """Backward of Conv+BN+ReLU+MaxPool(3,2,1) from the POOLED output's gradient (the full-resolution gradient is gathered on
    the fly, never stored). -> dz, dgamma, dbeta."""
    n, h, w, c = z.shape
    dz, dgamma, dbeta, coef = _bn_bwd_outs(z, dgamma, dbeta)
    _check(lib().vatl_bn_train_bwd_relu_pool(_ptr(dpool), _ptr(idx, torch.uint8), _ptr(scale), _ptr(bias), _ptr(z), _ptr(gamma), _ptr(save_mean),
                                             _ptr(save_invstd), _ptr(dz), _ptr(dgamma), _ptr(dbeta), n, h, w, c, _ptr(coef),
                                             _ptr(_col_ws(n * h * w, c, z.device), torch.float64), _stream()), "vatl_bn_train_bwd_relu_pool")
    return dz, dgamma, dbeta


def maxpool3x3s2_bwd(x, dy):
    n, h, w, c = x.shape
    dx = torch.empty_like(x)
    _check(lib().vatl_maxpool3x3s2_bwd(_ptr(x), _ptr(dy), _ptr(dx), n, h, w, c, _stream()), "vatl_maxpool3x3s2_bwd")
    return dx


def maxpool3x3s2_bwd_idx(dy, idx, in_hw):
    n, _, _, c = dy.shape
    dx = torch.empty((n, in_hw[0], in_hw[1], c), device=dy.device, dtype=torch.float32)
    _check(lib().vatl_maxpool3x3s2_bwd_idx(_ptr(dy), _ptr(idx, torch.uint8), _ptr(dx), n, in_hw[0], in_hw[1], c, _stream()), "vatl_maxpool3x3s2_bwd_idx")
    return dx


def pixelunshuffle2(x):
    n, h2, w2, c4 = x.shape
    y = torch.empty((n, h2 // 2, w2 // 2, c4 * 4), device=x.device, dtype=torch.float32)
    _check(lib().vatl_pixelunshuffle2(_ptr(x), _ptr(y), n, h2 // 2, w2 // 2, c4 * 4, _stream()), "vatl_pixelunshuffle2")
    return y


def upsample_nearest_bwd(dy, yact, shift: int):
    """dy (N,H,W,C) [masked by yact > 0] -> block sums (N,H>>shift,W>>shift,C)."""
    n, h, w, c = dy.shape
    dz = torch.empty((n, h >> shift, w >> shift, c), device=dy.device, dtype=torch.float32)
    _check(lib().vatl_upsample_nearest_bwd(_ptr(dy), _ptr(yact), _ptr(dz), n, h, w, c, shift, _stream()), "vatl_upsample_nearest_bwd")
    return dz


def gap_bwd(dy, hw: int):
    n, c = dy.shape
    dx = torch.empty((n, hw, c), device=dy.device, dtype=torch.float32)
    _check(lib().vatl_gap_bwd(_ptr(dy), _ptr(dx), n, hw, c, _stream()), "vatl_gap_bwd")
    return dx


def se_bwd_gate(dy, y, u, gate):
    n, h, w, c = dy.shape
    dgate = torch.empty((n, c), device=dy.device, dtype=torch.float32)
    _check(lib().vatl_se_bwd(_ptr(dy), _ptr(y), _ptr(u), _ptr(gate), None, _ptr(dgate), None, None, n, h * w, c, _stream()), "vatl_se_bwd")
    return dgate


def se_bwd_apply(dy, y, gate, dpool):
    n, h, w, c = dy.shape
    du, gm = torch.empty_like(dy), torch.empty_like(dy)
    _check(lib().vatl_se_bwd(_ptr(dy), _ptr(y), None, _ptr(gate), _ptr(dpool), None, _ptr(du), _ptr(gm), n, h * w, c, _stream()), "vatl_se_bwd")
    return du, gm


def relu_bwd(dy, y):
    dx = torch.empty_like(dy)
    _check(lib().vatl_relu_bwd(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), _stream()), "vatl_relu_bwd")
    return dx


def col_sum(x2d):
    c = x2d.shape[-1]
    m = x2d.numel() // c
    out = torch.empty(c, device=x2d.device, dtype=torch.float32)
    _check(lib().vatl_col_sum(_ptr(x2d), m, c, _ptr(out), _ptr(_col_ws(m, c, x2d.device), torch.float64), _stream()), "vatl_col_sum")
    return out


# ----------------------------------------------------------------------------
# deformable 3x3 convolution (DCN v1 / v2), csrc/deform_conv.hip
# ----------------------------------------------------------------------------

def deform_conv2d_supported(c: int, cout: int, stride: int, dg: int) -> bool:
    return bool(lib().vatl_deform_conv2d_supported(c, cout, stride, dg))


def pack_deform_weight(w: torch.Tensor) -> torch.Tensor:
    """(Cout,C,3,3) -> [tap][C][Cout], the filter layout of the fused deformable forward."""
    cout, c, r, s = w.shape
    if (r, s) != (3, 3):
        raise VatlError("deformable convolutions are 3x3")
    return w.detach().permute(2, 3, 1, 0).contiguous().view(9, c, cout)


def deform_col_stride(c: int) -> int:
    """Row length of the column matrix: 9 * C rounded up to the 32-float K step of the GEMMs that read it."""
    return (9 * c + 31) // 32 * 32


def deform_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """(Cout,C,3,3) -> (Cout,K,1,1) with K = deform_col_stride(C), column t * C + c (zeros behind 9 * C): the filter as the 1x1 conv that
    multiplies the column matrix."""
    cout, c = w.shape[:2]
    k = deform_col_stride(c)
    out = torch.zeros((cout, k, 1, 1), device=w.device, dtype=torch.float32)
    out[:, :9 * c, 0, 0] = w.detach().permute(0, 2, 3, 1).reshape(cout, 9 * c)
    return out


def _deform_args(who: str, x, offset, mask, stride: int, dg: int, mask_logits: bool):
    """Geometry and the (offset, mask) pointer arguments of the deformable entry points.  ``offset`` (N,Ho,Wo,>= 18 dg) NHWC; ``mask`` is
    None (DCN v1), a (N,Ho,Wo,>= 9 dg) tensor, or True: the mask logits follow the offsets inside ``offset`` (conv2_offset's output)."""
    n, h, w, c = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if tuple(offset.shape[:3]) != (n, ho, wo) or offset.shape[3] < (27 if mask is True else 18) * dg:
        raise VatlError(f"{who}: offset tensor {tuple(offset.shape)} does not fit x {tuple(x.shape)}, stride {stride}, {dg} deformable groups")
    optr = _ptr(offset)
    if mask is None:
        margs = (None, 0, 0)
    elif mask is True:
        margs = (optr + 72 * dg, offset.shape[3], 1)
    else:
        if tuple(mask.shape[:3]) != (n, ho, wo) or mask.shape[3] < 9 * dg:
            raise VatlError(f"{who}: mask tensor {tuple(mask.shape)} does not fit")
        margs = (_ptr(mask), mask.shape[3], int(mask_logits))
    return (n, h, w, c, ho, wo), (optr, offset.shape[3]) + margs


def deform_conv2d_fwd(x, w_tcc, offset, mask, scale, bias, stride: int, dg: int, relu: bool, mask_logits: bool = False, out=None):
    """Fused deformable conv + folded scale / bias (+ ReLU): x (N,H,W,C) NHWC, w_tcc from pack_deform_weight -> (N,Ho,Wo,Cout)."""
    (n, h, w, c, ho, wo), oargs = _deform_args("deform_conv2d_fwd", x, offset, mask, stride, dg, mask_logits)
    cout = w_tcc.shape[2]
    if tuple(w_tcc.shape) != (9, c, cout):
        raise VatlError(f"deform_conv2d_fwd: filter {tuple(w_tcc.shape)} for {c} input channels")
    y = out if out is not None else torch.empty((n, ho, wo, cout), device=x.device, dtype=torch.float32)
    if tuple(y.shape) != (n, ho, wo, cout):
        raise VatlError("deform_conv2d_fwd: out has the wrong shape")
    _check(lib().vatl_deform_conv2d_fwd(_ptr(x), _ptr(w_tcc), *oargs, _ptr(scale), _ptr(bias), _ptr(y), n, h, w, c, cout, stride, dg, int(relu),
                                        _stream()), "vatl_deform_conv2d_fwd")
    return y


def deform_columns(x, offset, mask, stride: int, dg: int, mask_logits: bool = False):
    """The sampled, mask-weighted column matrix (N,Ho,Wo,deform_col_stride(C)), column t * C + c."""
    (n, h, w, c, ho, wo), oargs = _deform_args("deform_columns", x, offset, mask, stride, dg, mask_logits)
    k = deform_col_stride(c)
    col = torch.empty((n, ho, wo, k), device=x.device, dtype=torch.float32)
    _check(lib().vatl_deform_columns(_ptr(x), *oargs, _ptr(col), k, n, h, w, c, stride, dg, _stream()), "vatl_deform_columns")
    return col


# Process switch of the deformable backward's dx (public face: alphapose.models.layers.dcn.set_deterministic / is_deterministic /
# deterministic): True = the ordered, bit-reproducible entry, False = float atomics, None (the default) = follow torch.
_deform_deterministic = None


def set_deform_deterministic(mode):
    global _deform_deterministic
    if mode not in (True, False, None):
        raise ValueError(f"deterministic mode {mode!r}: True, False or None (follow torch)")
    _deform_deterministic = mode


def deform_deterministic_mode():
    """The switch as it was set: True, False or None."""
    return _deform_deterministic


def deform_deterministic() -> bool:
    """The switch resolved now: with None the ordered path is on when torch.are_deterministic_algorithms_enabled() or
    torch.backends.cudnn.deterministic is."""
    if _deform_deterministic is None:
        return bool(torch.are_deterministic_algorithms_enabled() or torch.backends.cudnn.deterministic)
    return _deform_deterministic


def deform_dx_index_bytes(n: int, h: int, w: int, stride: int, dg: int) -> int:
    """Workspace bytes of the ordered dx (the inverted index): include/vatl_hip.h states the formula."""
    b = int(lib().vatl_deform_dx_index_bytes(n, h, w, stride, dg))
    if b < 0:
        _check(b, "vatl_deform_dx_index_bytes")
    return b


def deform_columns_bwd(dcol, x, offset, mask, stride: int, dg: int, mask_logits: bool = False, grad_channels: int | None = None,
                       deterministic: bool | None = None):
    """Backward of deform_columns -> (dx, d_offset, d_mask).  d_offset is (N,Ho,Wo,grad_channels or offset's channel count), zero
    behind the gradients; with ``mask is True`` the logit gradients follow the offset gradients inside it (the layout of ``offset``) and
    d_mask is None.  ``deterministic``: False = dx from float atomics (equal in value from run to run, not in bits); True = the ordered
    entry, whose dx has the same bits on every run (its index workspace comes from torch's allocator, per call: stream-safe); None =
    the process switch (``deform_deterministic()``).  d_offset and d_mask have the same bits either way."""
    (n, h, w, c, ho, wo), oargs = _deform_args("deform_columns_bwd", x, offset, mask, stride, dg, mask_logits)
    k = deform_col_stride(c)
    if tuple(dcol.shape) != (n, ho, wo, k):
        raise VatlError(f"deform_columns_bwd: dcol {tuple(dcol.shape)}, expected {(n, ho, wo, k)}")
    gc = grad_channels or offset.shape[3]
    if gc < (27 if mask is True else 18) * dg:
        raise VatlError("deform_columns_bwd: grad_channels too small")
    if deterministic is None:
        deterministic = deform_deterministic()
    dx = torch.empty_like(x)
    d_off = torch.zeros((n, ho, wo, gc), device=x.device, dtype=torch.float32)
    d_mask = None
    if mask is True:
        dm = (_ptr(d_off) + 72 * dg, gc)
    elif mask is not None:
        d_mask = torch.empty((n, ho, wo, 9 * dg), device=x.device, dtype=torch.float32)
        dm = (_ptr(d_mask), 9 * dg)
    else:
        dm = (None, 0)
    args = (_ptr(dcol), k, _ptr(x), *oargs, _ptr(dx), _ptr(d_off), gc, *dm, n, h, w, c, stride, dg)
    if deterministic:
        ws = torch.empty(deform_dx_index_bytes(n, h, w, stride, dg), device=x.device, dtype=torch.uint8)
        _check(lib().vatl_deform_columns_bwd_ordered(*args, _ptr(ws, torch.uint8), ws.numel(), _stream()), "vatl_deform_columns_bwd_ordered")
    else:
        _check(lib().vatl_deform_columns_bwd(*args, _stream()), "vatl_deform_columns_bwd")
    return dx, d_off, d_mask


# ----------------------------------------------------------------------------
# fine-tune step pieces
# ----------------------------------------------------------------------------

def masked_mse_fwd_bwd(out: torch.Tensor, target: torch.Tensor, mask: torch.Tensor):
    """-> loss (1,) f32 on device, grad like ``out``."""
    n, j, h, w = out.shape
    grad = torch.empty_like(out)
    loss = torch.empty(1, device=out.device, dtype=torch.float32)
    ws = torch.empty(int(lib().vatl_masked_mse_workspace_floats(out.numel())), device=out.device, dtype=torch.float32)
    m = mask.reshape(n, j).contiguous()
    _check(lib().vatl_masked_mse_fwd_bwd(_ptr(out), _ptr(target), _ptr(m), _ptr(grad), _ptr(loss), _ptr(ws), n, j, h * w, _stream()),
           "vatl_masked_mse_fwd_bwd")
    return loss, grad


NORM_TYPES = {"softmax": 0, "sigmoid": 1, "divide_sum": 2}


def l1_joint_regression_fwd_bwd(hm, gt_joints, gt_joints_vis, norm_type: str = "softmax", size_average: bool = True):
    """-> loss (0-dim), grad (B,J,H,W), pred_jts (B,2J)."""
    b, j, h, w = hm.shape
    grad = torch.empty_like(hm)
    loss = torch.empty((), device=hm.device, dtype=torch.float32)
    jts = torch.empty((b, 2 * j), device=hm.device, dtype=torch.float32)
    partial = torch.empty(b * j, device=hm.device, dtype=torch.float64)
    _check(lib().vatl_l1_joint_regression_fwd_bwd(_ptr(hm), _ptr(gt_joints), _ptr(gt_joints_vis), _ptr(grad), _ptr(loss), _ptr(jts),
                                                  _ptr(partial, torch.float64), b, j, h, w, NORM_TYPES[norm_type], int(size_average), _stream()),
           "vatl_l1_joint_regression_fwd_bwd")
    return loss, grad, jts


def gaussian_targets(joints_xy, vis, hm_hw=(64, 48), in_hw=(256, 192), sigma: float = 2.0):
    """joints (N,J,2) input-pixel coordinates, vis (N,J) -> target (N,J,H,W), weight (N,J,1,1)  [_target_generator]."""
    n, j, _ = joints_xy.shape
    target = torch.empty((n, j, hm_hw[0], hm_hw[1]), device=joints_xy.device, dtype=torch.float32)
    weight = torch.empty((n, j), device=joints_xy.device, dtype=torch.float32)
    _check(lib().vatl_gaussian_targets(_ptr(joints_xy.contiguous()), _ptr(vis.contiguous()), _ptr(target), _ptr(weight), n, j, hm_hw[0], hm_hw[1],
                                       in_hw[0], in_hw[1], sigma, _stream()), "vatl_gaussian_targets")
    return target, weight.reshape(n, j, 1, 1)


PIXEL_MEAN = (0.406, 0.457, 0.480)          # simple_transform.py:93-95


def crop_warp_affine(arena, src_off, src_hwf, minv, out_hw=(256, 192), mean=PIXEL_MEAN, out=None):
    """cv2.warpAffine(INTER_LINEAR) + im_to_torch + mean shift for B crops in one call  [SimpleTransform.test_transform].

    arena: uint8 device tensor holding the packed (h, w, 3) frames; src_off (B,) int64 byte offsets; src_hwf (B,3) int32
    {h, w, mirror}; minv (B,2,3) float64 dst->src maps.  Returns (B,3,out_h,out_w) fp32 and the per-crop u8 maxima."""
    b = int(src_off.shape[0])
    dev = arena.device
    if out is None:
        out = torch.empty((b, 3, out_hw[0], out_hw[1]), device=dev, dtype=torch.float32)
    cmax = torch.empty(b, device=dev, dtype=torch.int32)
    _check(lib().vatl_crop_warp_affine(_ptr(arena, torch.uint8), _ptr(src_off, torch.int64), _ptr(src_hwf.contiguous(), torch.int32),
                                       _ptr(minv.contiguous(), torch.float64), _ptr(out), _ptr(cmax, torch.int32), b, out_hw[0], out_hw[1],
                                       float(mean[0]), float(mean[1]), float(mean[2]), _stream()),
           "vatl_crop_warp_affine")
    return out, cmax


# ----------------------------------------------------------------------------
# hybrid JPEG decoder: Huffman pass on the host, pixels on the device
# ----------------------------------------------------------------------------

JPEG_DESC_INTS = 16                     # include/vatl_hip.h: the frame descriptor
JPEG_REFUSALS = ("admitted", "not_jpeg", "bad_header", "not_baseline", "precision", "components", "sampling", "too_small", "multiple_scans",
                 "colour_space", "quant_precision", "too_large", "segment_too_long")          # VATL_JPEG_* codes of include/vatl_hip.h, in order (tests/test_jpeg_tables.py)
JPEG_TABLE_COLS = 12                    # csrc/jpeg.hip: one int64 row per frame of a batch


class JpegInfo:
    """What `jpeg_probe` says about a stream: ``admitted`` (the device path decodes it) or not, with ``reason`` (the refusal's name,
    one of JPEG_REFUSALS) and ``detail`` (its text); for streams whose frame header was read also height, width, components,
    ``sampling`` ("gray" / "4:4:4" / "4:2:0" / None), ``blocks`` per component and the coefficient count."""

    def __init__(self, desc, detail=""):
        d = [int(v) for v in desc]
        self.desc = desc
        self.admitted = bool(d[0])
        self.reason = JPEG_REFUSALS[d[1]] if 0 <= d[1] < len(JPEG_REFUSALS) else f"code_{d[1]}"
        self.detail = detail
        self.height, self.width, self.components = d[2], d[3], d[4]
        self.sampling = None if not d[5] else "gray" if d[4] == 1 else "4:4:4" if d[5] == 1 else "4:2:0"
        self.blocks = (d[8] * d[9],) + ((d[10] * d[11],) * 2 if d[4] == 3 else ())
        self.coefficients = 64 * d[12]
        self.restart_interval = d[13]

    def __repr__(self):
        what = "admitted" if self.admitted else f"refused: {self.reason} ({self.detail})"
        return f"JpegInfo({self.height}x{self.width}, {self.components} components, {self.sampling}, {what})"


class JpegCoefficients:
    """One frame after the host pass: ``coef`` int16 (64 * blocks,) host tensor — natural order, not dequantised, per component in
    block-raster order, pinned when a device is present —, ``qt`` (3, 64) uint16 quantiser tables per component, ``desc`` the descriptor."""

    def __init__(self, coef, qt, desc):
        self.coef, self.qt, self.desc = coef, qt, desc
        self.height, self.width, self.blocks = int(desc[2]), int(desc[3]), int(desc[12])


def _host_bytes(data):
    import numpy as np
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)
    if a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise VatlError("a JPEG stream is bytes (or a contiguous 1-D uint8 array)")
    return a


def jpeg_probe(data) -> JpegInfo:
    """File bytes -> JpegInfo.  Host only (works without a GPU); a stream the device path does not decode — progressive, 4:2:2,
    under 8 px, no JPEG at all — is refused with a reason, never an error."""
    import numpy as np
    a = _host_bytes(data)
    desc = np.zeros(JPEG_DESC_INTS, np.int32)
    _check(lib().vatl_jpeg_probe(a.ctypes.data, a.size, desc.ctypes.data), "vatl_jpeg_probe")
    return JpegInfo(desc, "" if desc[0] else lib().vatl_last_error().decode())


def jpeg_entropy_decode(data) -> JpegCoefficients:
    """File bytes of an ADMITTED stream -> JpegCoefficients.  Host only; the call releases the GIL, so a thread pool decodes in
    parallel.  Raises VatlError for a refused stream and for a truncated / corrupt one."""
    import numpy as np
    a = _host_bytes(data)
    info = jpeg_probe(a)
    if not info.admitted:
        raise VatlError(f"vatl_jpeg_entropy_decode: stream refused ({info.reason}): {info.detail}")
    coef = torch.empty(info.coefficients, dtype=torch.int16, pin_memory=torch.cuda.is_available())
    qt = np.zeros((3, 64), np.uint16)
    desc = np.zeros(JPEG_DESC_INTS, np.int32)
    _check(lib().vatl_jpeg_entropy_decode(a.ctypes.data, a.size, coef.data_ptr(), coef.numel(), qt.ctypes.data, desc.ctypes.data), "vatl_jpeg_entropy_decode")
    return JpegCoefficients(coef, qt, desc)


def jpeg_decode_batch(frames, device=None, out=None, marks=None):
    """Coefficient frames of a whole batch -> pixels, in ONE call (two launches): returns (data, offsets, hw) in FrameArena's layout —
    ``data`` a uint8 device tensor with the frames as packed (h, w, 3) RGB back to back, ``offsets`` (n,) int64 byte offsets,
    ``hw`` (n, 2) int32.  ``out``: a uint8 device tensor of at least sum(h * w * 3) bytes to write into (nothing past that sum is touched).
    ``marks``: a list that receives three timing events of the stream — before the uploads, between uploads and launches, after the
    launches (tools/jpeg_decode_bench.py splits the call's device time with them)."""
    import numpy as np
    frames = list(frames)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise VatlError("jpeg_decode_batch writes a device arena; there is no CPU path")
    n = len(frames)
    hw = np.array([[f.height, f.width] for f in frames], np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    ends = np.cumsum(sizes)
    offsets = (ends - sizes).astype(np.int64)
    total = int(ends[-1]) if n else 0
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=device)
    elif not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < total or not out.is_contiguous():
        raise VatlError(f"jpeg_decode_batch: `out` must be a contiguous 1-D uint8 device tensor of >= {total} bytes")
    if n == 0:
        return out, offsets, hw
    table = np.zeros((n + 1, JPEG_TABLE_COLS), np.int64)
    blocks = np.array([f.blocks for f in frames], np.int64)
    groups = ((offsets & 3) + sizes + 11) // 12
    table[1:, 0], table[1:, 1] = np.cumsum(blocks), np.cumsum(groups)
    table[:n, 2] = offsets
    for k, f in enumerate(frames):
        d = f.desc
        table[k, 3:11] = (d[2], d[3], d[4], d[5], d[8], d[9], d[10], d[11])
    nblocks, ngroups = int(table[n, 0]), int(table[n, 1])
    def mark():
        if marks is not None:
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()
    with torch.cuda.device(device):
        coef = torch.empty(nblocks * 64, dtype=torch.int16, device=device)
        mark()
        for k, f in enumerate(frames):
            if f.coef.numel() != 64 * f.blocks:
                raise VatlError("jpeg_decode_batch: a frame's coefficient count does not match its descriptor")
            coef[int(table[k, 0]) * 64:int(table[k + 1, 0]) * 64].copy_(f.coef, non_blocking=True)
        qt = upload(np.stack([f.qt for f in frames]).view(np.int16), device)
        tab = upload(table, device)
        planes = torch.empty(nblocks * 64, dtype=torch.uint8, device=device)
        mark()
        _check(lib().vatl_jpeg_pixels(_ptr(coef, torch.int16), _ptr(qt, torch.int16), _ptr(tab, torch.int64), n, nblocks, ngroups,
                                      _ptr(planes, torch.uint8), _ptr(out, torch.uint8), total, _stream()), "vatl_jpeg_pixels")
        mark()
    return out, offsets, hw


# ----------------------------------------------------------------------------
# Huffman decoding on the device: the host only packs the stream
# ----------------------------------------------------------------------------

JPEG_SUB_BYTES = 128                    # include/vatl_hip.h VATL_JHUFF_*: one lane's share of a scan,
JPEG_BLOCK_SUBS = 256                   # lanes per thread block,
JPEG_HUFF_BYTES = 8544                  # a frame's six Huffman tables,
JPEG_HUFF_TABLE_COLS = 16               # one int64 row per frame of a batch,
JPEG_HUFF_ACTIVE_WORDS = 64             # the workspace's last words: thread blocks that worked in each synchronisation launch
JPEG_HUFFMAN_STATUS = ("ok", "bad_dc_code", "bad_ac_code", "zero_run_past_63", "data_ends_early", "blocks_short", "restart_marker_unread")


class JpegPacked:
    """One frame after `jpeg_pack`: ``scan`` uint8 host tensor — the entropy-coded data without byte stuffing, cut at the restart markers,
    each segment padded to whole 128-byte subsequences; pinned when a device is present —, ``segments`` (n, 4) int32 rows {byte offset in
    scan, real bit length, first MCU, MCU count}, ``huff`` the frame's Huffman tables as the kernels probe them (JPEG_HUFF_BYTES uint8),
    ``qt`` (3, 64) uint16 and ``desc`` as `jpeg_entropy_decode` gives them."""

    def __init__(self, scan, segments, huff, qt, desc):
        self.scan, self.segments, self.huff, self.qt, self.desc = scan, segments, huff, qt, desc
        self.height, self.width, self.blocks = int(desc[2]), int(desc[3]), int(desc[12])


def jpeg_pack(data) -> JpegPacked:
    """File bytes of an ADMITTED stream -> JpegPacked: everything the host still does when the Huffman pass runs on the device.  Host
    only; the call releases the GIL.  Raises VatlError for a refused stream (what `jpeg_probe` refuses, and a stream with more than
    768 KiB between restart markers: "segment_too_long"), for an undefined table and for a missing or misnumbered restart marker."""
    import numpy as np
    a = _host_bytes(data)
    cap = np.zeros(2, np.int64)
    if lib().vatl_jpeg_pack_size(a.ctypes.data, a.size, cap[0:].ctypes.data, cap[1:].ctypes.data) != 0:
        info = jpeg_probe(a)
        raise VatlError(f"vatl_jpeg_pack: stream refused ({info.reason}): {info.detail}")
    scan = torch.empty(int(cap[0]), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    segments = np.zeros((int(cap[1]), 4), np.int32)
    huff, qt, desc, used = np.zeros(JPEG_HUFF_BYTES, np.uint8), np.zeros((3, 64), np.uint16), np.zeros(JPEG_DESC_INTS, np.int32), np.zeros(2, np.int64)
    rc = lib().vatl_jpeg_pack(a.ctypes.data, a.size, scan.data_ptr(), scan.numel(), segments.ctypes.data, segments.shape[0], huff.ctypes.data, qt.ctypes.data,
                              desc.ctypes.data, used.ctypes.data)
    if rc != 0 and not desc[0] and 0 < desc[1] < len(JPEG_REFUSALS):
        raise VatlError(f"vatl_jpeg_pack: stream refused ({JPEG_REFUSALS[desc[1]]}): {lib().vatl_last_error().decode()}")
    _check(rc, "vatl_jpeg_pack")
    return JpegPacked(scan[:int(used[0])], segments[:int(used[1])], huff, qt, desc)


def jpeg_huffman_batch(frames, device=None, marks=None, stats=None, coef=None):
    """Packed frames of a whole batch -> their coefficients on the device, Huffman-decoded there: returns (coef, table, status) —
    ``coef`` an int16 device tensor with every frame's coefficients back to back in `jpeg_entropy_decode`'s layout, ``table`` the
    (n + 1, JPEG_HUFF_TABLE_COLS) int64 host table (column 4: a frame's first coefficient block), ``status`` an (n,) int32 DEVICE tensor
    — 0, or an index into JPEG_HUFFMAN_STATUS for a stream the host decoder rejects too.  ``marks`` receives timing events like
    `jpeg_decode_batch`'s; ``stats``: a dict that receives "launches" and, read back (a synchronisation), "active_blocks" per launch;
    ``coef``: an int16 device tensor of at least 64 * sum(blocks) elements to decode into (nothing past that count is touched)."""
    import numpy as np
    frames = list(frames)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise VatlError("jpeg_huffman_batch decodes on the device; there is no CPU path")
    n = len(frames)
    if n == 0:
        raise VatlError("jpeg_huffman_batch: no frames")
    block_bytes = JPEG_SUB_BYTES * JPEG_BLOCK_SUBS
    table = np.zeros((n + 1, JPEG_HUFF_TABLE_COLS), np.int64)
    launches = 1
    for k, f in enumerate(frames):
        d, subs = f.desc, f.scan.numel() // JPEG_SUB_BYTES
        if f.scan.numel() != subs * JPEG_SUB_BYTES or subs == 0 or f.segments.shape[0] == 0 or f.huff.size != JPEG_HUFF_BYTES:
            raise VatlError("jpeg_huffman_batch: a frame is not what jpeg_pack returns")
        table[k, 1], table[k, 3] = subs, f.segments.shape[0]
        table[k, 5:14] = (d[12], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11])
        table[k + 1, 0] = table[k, 0] + -(-subs // JPEG_BLOCK_SUBS)
        table[k + 1, 2] = table[k, 2] + f.segments.shape[0]
        table[k + 1, 4] = table[k, 4] + int(d[12])
        first = f.segments[:, 0].astype(np.int64) // JPEG_SUB_BYTES                  # a segment's first and last subsequence -> the thread blocks it spans
        last = np.append(first[1:], subs) - 1
        launches = max(launches, int((last // JPEG_BLOCK_SUBS - first // JPEG_BLOCK_SUBS).max()) + 1)
    tbs, nseg, nblocks = int(table[n, 0]), int(table[n, 2]), int(table[n, 4])
    def mark():
        if marks is not None:
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()
    with torch.cuda.device(device):
        scan = torch.empty(tbs * block_bytes, dtype=torch.uint8, device=device)
        mark()
        for k, f in enumerate(frames):
            at = int(table[k, 0]) * block_bytes
            scan[at:at + f.scan.numel()].copy_(f.scan, non_blocking=True)
        segs = upload(np.concatenate([f.segments for f in frames]), device)
        huff = upload(np.concatenate([f.huff for f in frames]), device)
        tab = upload(table, device)
        if coef is None:
            coef = torch.empty(nblocks * 64, dtype=torch.int16, device=device)
        elif not coef.is_cuda or coef.dtype != torch.int16 or coef.dim() != 1 or coef.numel() < nblocks * 64 or not coef.is_contiguous():
            raise VatlError(f"jpeg_huffman_batch: `coef` must be a contiguous 1-D int16 device tensor of >= {nblocks * 64} elements")
        status = torch.empty(n, dtype=torch.int32, device=device)
        need = int(lib().vatl_jpeg_huffman_workspace_bytes(tbs, nseg))
        if need <= 0:
            raise VatlError(f"jpeg_huffman_batch: a batch of {tbs} thread blocks and {nseg} segments is out of range")
        ws = torch.empty(need // 4, dtype=torch.int32, device=device)
        mark()
        _check(lib().vatl_jpeg_huffman(_ptr(scan, torch.uint8), _ptr(segs, torch.int32), _ptr(huff, torch.uint8), _ptr(tab, torch.int64), n, tbs, nseg, launches,
                                       _ptr(coef, torch.int16), nblocks * 64, _ptr(status, torch.int32), _ptr(ws, torch.int32), need, _stream()), "vatl_jpeg_huffman")
        mark()
        if stats is not None:
            stats["launches"] = launches
            stats["active_blocks"] = ws[-JPEG_HUFF_ACTIVE_WORDS:][:min(launches, JPEG_HUFF_ACTIVE_WORDS)].tolist()
    return coef, table, status


def jpeg_decode_packed_batch(frames, device=None, out=None, marks=None, stats=None):
    """`jpeg_decode_batch` for JpegPacked frames: Huffman decoding (`jpeg_huffman_batch`) and the pixel stage in one go, nothing read
    back.  Returns (data, offsets, hw, status): the first three as `jpeg_decode_batch`, ``status`` the (n,) int32 device tensor of
    `jpeg_huffman_batch` — the pixels of a frame whose status is not 0 mean nothing (the caller decodes that file another way).
    ``marks`` receives five events: before the uploads, before the Huffman launches, after them, before and after the pixel launches."""
    import numpy as np
    frames = list(frames)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n = len(frames)
    hw = np.array([[f.height, f.width] for f in frames], np.int32).reshape(-1, 2)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    ends = np.cumsum(sizes)
    offsets = (ends - sizes).astype(np.int64)
    total = int(ends[-1]) if n else 0
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=device)
    elif not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < total or not out.is_contiguous():
        raise VatlError(f"jpeg_decode_packed_batch: `out` must be a contiguous 1-D uint8 device tensor of >= {total} bytes")
    if n == 0:
        return out, offsets, hw, torch.empty(0, dtype=torch.int32, device=device)
    coef, htable, status = jpeg_huffman_batch(frames, device, marks, stats)
    table = np.zeros((n + 1, JPEG_TABLE_COLS), np.int64)
    groups = ((offsets & 3) + sizes + 11) // 12
    table[:, 0], table[1:, 1] = htable[:, 4], np.cumsum(groups)
    table[:n, 2] = offsets
    for k, f in enumerate(frames):
        d = f.desc
        table[k, 3:11] = (d[2], d[3], d[4], d[5], d[8], d[9], d[10], d[11])
    nblocks, ngroups = int(table[n, 0]), int(table[n, 1])
    with torch.cuda.device(device):
        qt = upload(np.stack([f.qt for f in frames]).view(np.int16), device)
        tab = upload(table, device)
        planes = torch.empty(nblocks * 64, dtype=torch.uint8, device=device)
        if marks is not None:
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()
        _check(lib().vatl_jpeg_pixels(_ptr(coef, torch.int16), _ptr(qt, torch.int16), _ptr(tab, torch.int64), n, nblocks, ngroups,
                                      _ptr(planes, torch.uint8), _ptr(out, torch.uint8), total, _stream()), "vatl_jpeg_pixels")
        if marks is not None:
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()
    return out, offsets, hw, status


def ae_train_step(ae_flat, m, v, feat, d: int, z: int, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """One Adam step of the packed WholeBodyAE on the mini-batch feat (B, d); returns the loss (0-dim tensor)."""
    loss = torch.empty((), device=feat.device, dtype=torch.float32)
    _check(lib().vatl_ae_train_step(_ptr(ae_flat), _ptr(m), _ptr(v), _ptr(feat), feat.shape[0], d, z, lr, betas[0], betas[1], eps, step,
                                    _ptr(loss), _stream()), "vatl_ae_train_step")
    return loss


def ae_grad_workspace(n: int, d: int, z: int, device) -> torch.Tensor:
    """Block-partial workspace of ``ae_backward`` / ``ae_train_step_large`` for a batch of ``n`` rows (reusable across calls of that shape)."""
    floats = int(lib().vatl_ae_grad_workspace_floats(n, d, z))
    if floats <= 0:
        raise VatlError(f"auto-encoder batch {n} x {d} (z = {z}) is out of range: N >= 1, widths in 1..64")
    return torch.empty(floats, device=device, dtype=torch.float32)


def ae_backward(feat, dy, ae_flat, d: int, z: int, need_dx: bool = False, workspace=None):
    """Gradients of the packed WholeBodyAE for upstream gradients dy (N, d) at the input feat (N, d): (grad (P,), dx (N, d) or None)."""
    n = feat.shape[0]
    ws = workspace if workspace is not None else ae_grad_workspace(n, d, z, feat.device)
    grad = torch.empty_like(ae_flat)
    dx = torch.empty((n, d), device=feat.device, dtype=torch.float32) if need_dx else None
    _check(lib().vatl_ae_backward(_ptr(feat), _ptr(dy), _ptr(ae_flat), d, z, n, _ptr(grad), _ptr(dx), _ptr(ws), _stream()), "vatl_ae_backward")
    return grad, dx


def ae_train_step_large(ae_flat, m, v, feat, d: int, z: int, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                        weight_decay: float = 0.01, decoupled: bool = True, workspace=None, loss=None):
    """One AdamW (``decoupled``) or Adam step of the packed WholeBodyAE on feat (N, d), any N; returns the loss (0-dim tensor, or ``loss``
    when the caller gives a 1-element tensor to write into)."""
    n = feat.shape[0]
    ws = workspace if workspace is not None else ae_grad_workspace(n, d, z, feat.device)
    if loss is None:
        loss = torch.empty((), device=feat.device, dtype=torch.float32)
    _check(lib().vatl_ae_train_step_large(_ptr(ae_flat), _ptr(m), _ptr(v), _ptr(feat), n, d, z, lr, betas[0], betas[1], eps, weight_decay, step,
                                          int(bool(decoupled)), _ptr(loss), _ptr(ws), _stream()), "vatl_ae_train_step_large")
    return loss


def unpack_ae(flat: torch.Tensor, module) -> None:
    """Inverse of pack_ae: copy the packed parameters back into the encoder / decoder Linear layers."""
    off = 0
    with torch.no_grad():
        for half in (module.encoder, module.decoder):
            for i in (0, 2, 4, 6):
                for t in (half[i].weight, half[i].bias):
                    t.copy_(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()


class ChecksumTable:
    """Device table for vatl_checksum_multi over a fixed list of tensors (built once: their storage does not move while a plan lives)."""

    def __init__(self, tensors):
        bw = int(lib().vatl_checksum_block_words())
        rows, blocks = [], 0
        for t in tensors:
            if not (t.is_cuda and t.is_contiguous()):
                raise VatlError("checksum: contiguous device tensors only")
            nbytes = t.numel() * t.element_size()
            if nbytes % 4 or t.data_ptr() % 4:
                raise VatlError(f"checksum: a tensor of {nbytes} bytes at {t.data_ptr():#x} is not made of aligned 32-bit words")
            rows.append((t.data_ptr(), nbytes // 4, blocks))
            blocks += max(1, (nbytes // 4 + bw - 1) // bw)
        self.n, self.blocks = len(rows), blocks
        self.device = tensors[0].device if tensors else None
        self.table = upload(torch.tensor(rows, dtype=torch.int64), self.device) if rows else None

    def launch(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """Enqueue the checksums of the tensors' CURRENT contents on the current stream -> (n,) int64 device tensor (the bits of the uint64 sums)."""
        if out is None:
            out = torch.empty((self.n,), dtype=torch.int64, device=self.device)
        if self.n:
            _check(lib().vatl_checksum_multi(_ptr(self.table, torch.int64), self.n, self.blocks, _ptr(out, torch.int64), _stream()), "vatl_checksum_multi")
        return out


_opt_tables = {}                                     # (device, pointers...) -> (device table, total blocks): the pointers of a group do not change


def _multi_table(what, params, grads, ms, vs):
    """The device table of a multi-tensor optimiser launch: rows of {p, g, m, v, numel, first_block} (``ms`` / ``vs`` None: that
    column is 0)."""
    key = [params[0].device.index]
    for k, (p_, g_) in enumerate(zip(params, grads)):
        m_ = ms[k] if ms is not None else None
        v_ = vs[k] if vs is not None else None
        for t in (p_, g_) + (() if v_ is None else (v_,)) + (() if m_ is None else (m_,)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise VatlError(f"{what} needs contiguous fp32 device tensors")
        key += [p_.data_ptr(), g_.data_ptr(), 0 if m_ is None else m_.data_ptr(), 0 if v_ is None else v_.data_ptr(), p_.numel()]
    key = tuple(key)
    hit = _opt_tables.get(key)
    if hit is None:                                  # built and uploaded once per (group, storage): no per-step host-to-device copy
        be = int(lib().vatl_adamw_multi_block_elems())
        rows, blocks = [], 0
        for k in range(len(params)):
            p_, g_, m_, v_, n = key[1 + 5 * k:6 + 5 * k]
            rows.append((p_, g_, m_, v_, n, blocks))
            blocks += (n + be - 1) // be
        if len(_opt_tables) > 64:
            _opt_tables.clear()
        hit = _opt_tables[key] = (torch.tensor(rows, dtype=torch.int64).to(params[0].device), blocks)
    return hit


def _step_multi(what, params, grads, ms, vs, *scalars):
    """One ``vatl_<what>`` launch over the table of the lists (nothing to do for empty lists)."""
    if not params:
        return
    table, blocks = _multi_table(what, params, grads, ms, vs)
    _check(getattr(lib(), "vatl_" + what)(_ptr(table, torch.int64), len(params), blocks, *scalars, _stream()), "vatl_" + what)


def adamw_step_multi(params, grads, ms, vs, step: int, lr: float, weight_decay: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """One launch for a list of tensors sharing hyper-parameters and step count."""
    _step_multi("adamw_step_multi", params, grads, ms, vs, lr, betas[0], betas[1], eps, weight_decay, step)


def adam_step_multi(params, grads, ms, vs, step: int, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8):
    """``adam_step`` (L2 weight decay) for a list of tensors in one launch; the same bits as the per-tensor calls."""
    _step_multi("adam_step_multi", params, grads, ms, vs, lr, betas[0], betas[1], eps, weight_decay, step)


def rmsprop_step(p, g, sq, lr: float, alpha: float = 0.99, eps: float = 1e-8, weight_decay: float = 0.0):
    """torch.optim.RMSprop (momentum 0, not centered) on one contiguous tensor; ``sq`` is the running square average."""
    _check(lib().vatl_rmsprop_step(_ptr(p), _ptr(g), _ptr(sq), p.numel(), lr, alpha, eps, weight_decay, _stream()), "vatl_rmsprop_step")


def rmsprop_step_multi(params, grads, sqs, lr: float, alpha: float = 0.99, eps: float = 1e-8, weight_decay: float = 0.0):
    """``rmsprop_step`` for a list of tensors in one launch; the same bits as the per-tensor calls."""
    _step_multi("rmsprop_step_multi", params, grads, None, sqs, lr, alpha, eps, weight_decay)


def adam_step(p, g, m, v, step: int, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8):
    _check(lib().vatl_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay, step, _stream()),
           "vatl_adam_step")


def sgd_step(p, g, buf, step: int, lr: float, momentum: float = 0.9, weight_decay: float = 0.0):
    _check(lib().vatl_sgd_step(_ptr(p), _ptr(g), _ptr(buf), p.numel(), lr, momentum, weight_decay, step, _stream()), "vatl_sgd_step")


def sgd_step_multi(params, grads, bufs, step: int, lr: float, momentum: float = 0.9, weight_decay: float = 0.0):
    """``sgd_step`` for a list of tensors at one step count in one launch; the same bits as the per-tensor calls."""
    _step_multi("sgd_step_multi", params, grads, bufs, None, lr, momentum, weight_decay, step)


def adamw_step(p, g, m, v, step: int, lr: float, weight_decay: float, betas=(0.9, 0.999), eps: float = 1e-8):
    _check(lib().vatl_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay, step, _stream()),
           "vatl_adamw_step")


# ----------------------------------------------------------------------------
# float64 reference forward (csrc/conv_f64.hip, csrc/glue_f64.hip): NHWC float64 tensors, any channel count
# ----------------------------------------------------------------------------

def _new_f64(shape, like):
    return torch.empty(shape, device=like.device, dtype=torch.float64)


def pack_conv_weight_f64(w: torch.Tensor) -> torch.Tensor:
    """(Cout,Cin,R,S) fp32 -> [Cout][R][S][Cin] float64 (exact)."""
    cout, cin, r, s = w.shape
    out = _new_f64((cout, r, s, cin), w)
    _check(lib().vatl_pack_conv_weight_f64(_ptr(w.contiguous()), _f64(out), cout, cin, r, s, _stream()), "vatl_pack_conv_weight_f64")
    return out


def pack_deconv_weight_f64(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) fp32 -> four 2x2 phase filters [4][Cout][2][2][Cin] float64 (exact)."""
    cin, cout, kh, kw = w.shape
    if (kh, kw) != (4, 4):
        raise VatlError(f"pack_deconv_weight_f64: a 4x4 filter is needed, got {kh}x{kw}")
    out = _new_f64((4, cout, 2, 2, cin), w)
    _check(lib().vatl_pack_deconv4x4s2_weight_f64(_ptr(w.contiguous()), _f64(out), cin, cout, _stream()), "vatl_pack_deconv4x4s2_weight_f64")
    return out


def conv2d_fwd_f64(x, w_packed, scale, bias, stride: int, pad: int, relu: bool, residual=None, out_nchw: bool = False, out=None):
    """x (N,H,W,Cin) float64, w_packed from pack_conv_weight_f64 -> (N,Ho,Wo,Cout) float64 (or NCHW)."""
    n, h, w, cin = x.shape
    cout, r, s, cin_w = w_packed.shape
    if cin_w != cin:
        raise VatlError(f"conv2d_fwd_f64: input has {cin} channels, the filter {cin_w}")
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    shape = (n, cout, ho, wo) if out_nchw else (n, ho, wo, cout)
    if out is None:
        out = _new_f64(shape, x)
    elif tuple(out.shape) != shape:
        raise VatlError(f"conv2d_fwd_f64: out has shape {tuple(out.shape)}, expected {shape}")
    if residual is not None and tuple(residual.shape) != shape:
        raise VatlError(f"conv2d_fwd_f64: residual has shape {tuple(residual.shape)}, expected {shape}")
    _check(lib().vatl_conv2d_fwd_f64(_f64(x), _f64(w_packed), _f64(scale), _f64(bias), _f64(residual), _f64(out), n, h, w, cin, cout, r, s, stride, pad,
                                     int(relu), int(out_nchw), _stream()), "vatl_conv2d_fwd_f64")
    return out


def deconv4x4s2_fwd_f64(x, w_packed, scale, bias, relu: bool):
    n, h, w, cin = x.shape
    cout = w_packed.shape[1]
    if w_packed.shape[-1] != cin:
        raise VatlError(f"deconv4x4s2_fwd_f64: input has {cin} channels, the filter {w_packed.shape[-1]}")
    y = _new_f64((n, 2 * h, 2 * w, cout), x)
    _check(lib().vatl_deconv4x4s2_fwd_f64(_f64(x), _f64(w_packed), _f64(scale), _f64(bias), _f64(y), n, h, w, cin, cout, int(relu), _stream()),
           "vatl_deconv4x4s2_fwd_f64")
    return y


def nchw_to_nhwc_f64(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W) fp32 or float64 -> (N,H,W,C) float64; fp32 converts exactly."""
    if x.dtype not in (torch.float32, torch.float64):
        raise VatlError(f"nchw_to_nhwc_f64: expected fp32 or float64, got {x.dtype}")
    n, c, h, w = x.shape
    y = _new_f64((n, h, w, c), x)
    _check(lib().vatl_nchw_to_nhwc_f64(_ptr(x, x.dtype), int(x.dtype == torch.float64), _f64(y), n, c, h, w, _stream()), "vatl_nchw_to_nhwc_f64")
    return y


def nhwc_to_nchw_f64(x: torch.Tensor) -> torch.Tensor:
    n, h, w, c = x.shape
    y = _new_f64((n, c, h, w), x)
    _check(lib().vatl_nhwc_to_nchw_f64(_f64(x), _f64(y), n, c, h, w, _stream()), "vatl_nhwc_to_nchw_f64")
    return y


def maxpool3x3s2_fwd_f64(x):
    n, h, w, c = x.shape
    y = _new_f64((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), x)
    _check(lib().vatl_maxpool3x3s2_fwd_f64(_f64(x), _f64(y), n, h, w, c, _stream()), "vatl_maxpool3x3s2_fwd_f64")
    return y


def gap_fwd_f64(x):
    n, h, w, c = x.shape
    y = _new_f64((n, c), x)
    _check(lib().vatl_gap_fwd_f64(_f64(x), _f64(y), n, h * w, c, _stream()), "vatl_gap_fwd_f64")
    return y


def pixelshuffle2_fwd_f64(x):
    n, h, w, c = x.shape
    y = _new_f64((n, 2 * h, 2 * w, c // 4), x)
    _check(lib().vatl_pixelshuffle2_fwd_f64(_f64(x), _f64(y), n, h, w, c, _stream()), "vatl_pixelshuffle2_fwd_f64")
    return y


def se_scale_add_relu_f64(x, gate, residual):
    n, h, w, c = x.shape
    if tuple(gate.shape) != (n, c) or residual.shape != x.shape:
        raise VatlError("se_scale_add_relu_f64: gate must be (N,C) and the residual shaped like x")
    y = torch.empty_like(x)
    _check(lib().vatl_se_scale_add_relu_f64(_f64(x), _f64(gate), _f64(residual), _f64(y), n, h * w, c, _stream()), "vatl_se_scale_add_relu_f64")
    return y


def fuse_upsample_add_f64(base, ups, relu: bool):
    """base (N,H,W,C); ups = [(z, shift)] with z (N,H>>shift,W>>shift,C), at most 3, added in list order."""
    n, h, w, c = base.shape
    if len(ups) > 3:
        raise VatlError("fuse_upsample_add_f64: at most three up-sampled sources")
    for z, sh in ups:
        if tuple(z.shape) != (n, h >> sh, w >> sh, c):
            raise VatlError(f"fuse_upsample_add_f64: source {tuple(z.shape)} does not match {tuple(base.shape)} >> {sh}")
    y = torch.empty_like(base)
    a = list(ups) + [(None, 0)] * (3 - len(ups))
    _check(lib().vatl_fuse_upsample_add_f64(_f64(base), _f64(a[0][0]), a[0][1], _f64(a[1][0]), a[1][1], _f64(a[2][0]), a[2][1], _f64(y),
                                            n, h, w, c, int(relu), _stream()), "vatl_fuse_upsample_add_f64")
    return y


# float64 reference gradients (csrc/wgrad_f64.hip, csrc/train_glue_f64.hip, the data-gradient launcher of csrc/conv_f64.hip)

def _wgrad_shapes(who: str, x, dz, cout: int, cin: int, r: int, s: int, stride: int, pad: int, transposed: bool, out, align: int, dtype):
    """The shape contract of conv2d_wgrad_{f64,h16} (channels stored in multiples of ``align``) -> (n, h, w) of x, the pixels m of the dz
    side, the stored rows and columns of the GEMM, and ``out`` (allocated as ``dtype`` in the parameter's shape where None)."""
    n, h, w, cx = x.shape
    cz = dz.shape[-1]
    cin_s, cout_s = -(-cin // align) * align, -(-cout // align) * align
    if cx != cin_s or cz != cout_s:
        raise VatlError(f"{who}: tensors carry {cx} / {cz} channels, the filter has {cin} / {cout}")
    if transposed:
        want, m, rows, cols, shape = (n, 2 * h, 2 * w, cout_s), n * h * w, cin_s, cout_s, (cin, cout, 4, 4)
    else:
        ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
        want, m, rows, cols, shape = (n, ho, wo, cout_s), n * ho * wo, cout_s, cin_s, (cout, cin, r, s)
    if tuple(dz.shape) != want:
        raise VatlError(f"{who}: dz has shape {tuple(dz.shape)}, expected {want}")
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=dtype)
    elif tuple(out.shape) != shape:
        raise VatlError(f"{who}: out has shape {tuple(out.shape)}, expected {shape}")
    return (n, h, w), m, rows, cols, out


def _dgrad_shapes(who: str, dz, w_dgrad, xshape, r: int, s: int, stride: int, pad: int, residual):
    """The shape contract of conv2d_dgrad_{f64,h16} -> (n, h, w, cin, cout), channels as stored."""
    n, h, w, cin = xshape
    cout = dz.shape[-1]
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    if tuple(dz.shape) != (n, ho, wo, cout) or w_dgrad.numel() != cin * r * s * cout:
        raise VatlError(f"{who}: dz {tuple(dz.shape)} / filter of {w_dgrad.numel()} elements do not match input {tuple(xshape)}")
    if residual is not None and tuple(residual.shape) != (n, h, w, cin):
        raise VatlError(f"{who}: residual has shape {tuple(residual.shape)}, expected {(n, h, w, cin)}")
    return n, h, w, cin, cout


def _maxpool_bwd_shapes(who: str, dpool, x):
    n, h, w, c = x.shape
    if tuple(dpool.shape) != (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c):
        raise VatlError(f"{who}: dpool has shape {tuple(dpool.shape)}")
    return n, h, w, c


def _bn_ws(m: int, c: int, device, kind: str):
    """The float64 row-block partials of the BatchNorm / column reductions of the ``kind`` ("f64", "h16") training glue."""
    return torch.empty(int(getattr(lib(), f"vatl_bn_{kind}_workspace_doubles")(m, c)), device=device, dtype=torch.float64)


def wgrad_f64_splits(m: int) -> int:
    return int(lib().vatl_wgrad_f64_splits(m))


def conv2d_wgrad_f64(x, dz, cout: int, cin: int, r: int, s: int, stride: int, pad: int, transposed: bool = False, out=None):
    """Weight gradient in float64: (cout,cin,r,s) from x (N,H,W,cin) and dz (N,Ho,Wo,cout); ``transposed``: ConvTranspose2d(4,2,1)
    with x its forward input and dz (N,2H,2W,cout) its output gradient -> (cin,cout,4,4)."""
    (n, h, w), m, rows, cols, out = _wgrad_shapes("conv2d_wgrad_f64", x, dz, cout, cin, r, s, stride, pad, transposed, out, 1, torch.float64)
    doubles = int(lib().vatl_conv2d_wgrad_f64_workspace_doubles(rows, cols, r, s, m))
    ws = _new_f64((doubles,), x)
    _check(lib().vatl_conv2d_wgrad_f64(_f64(x), _f64(dz), _f64(ws), doubles, n, h, w, cin, cout, r, s, stride, pad, int(transposed), _stream()),
           "vatl_conv2d_wgrad_f64")
    _check(lib().vatl_wgrad_f64_reduce(_f64(ws), _f64(out), m, cout, cin, r, s, int(transposed), _stream()), "vatl_wgrad_f64_reduce")
    return out


def pack_conv_weight_dgrad_f64(w: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """(Cout,Cin,R,S) fp32 -> the flat data-gradient filters of conv2d_dgrad_f64 (Cin*R*S*Cout doubles, exact)."""
    cout, cin, r, s = w.shape
    out = _new_f64((cin * r * s * cout,), w)
    _check(lib().vatl_pack_conv_weight_dgrad_f64(_ptr(w.contiguous()), _f64(out), cout, cin, r, s, stride, pad, _stream()), "vatl_pack_conv_weight_dgrad_f64")
    return out


def conv2d_dgrad_f64(dz, w_dgrad, xshape, r: int, s: int, stride: int, pad: int, residual=None):
    """dx (N,H,W,Cin) = data gradient of a (r x s, stride, pad) conv from dz (N,Ho,Wo,Cout); ``residual`` shaped like dx is added."""
    n, h, w, cin, cout = _dgrad_shapes("conv2d_dgrad_f64", dz, w_dgrad, xshape, r, s, stride, pad, residual)
    dx = _new_f64((n, h, w, cin), dz)
    _check(lib().vatl_conv2d_dgrad_f64(_f64(dz), _f64(w_dgrad), _f64(residual), _f64(dx), n, h, w, cin, cout, r, s, stride, pad, _stream()),
           "vatl_conv2d_dgrad_f64")
    return dx


def bn_train_fwd_stats_f64(z, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """z NHWC float64 -> (7,C) float64: batch mean, biased variance, invstd, scale, bias, and the running mean / unbiased running
    variance a training step WOULD write from ``running_mean`` / ``running_var`` (float64 copies; nothing is updated)."""
    c = z.shape[-1]
    m = z.numel() // c
    for name, t in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and t.numel() != c:
            raise VatlError(f"bn_train_fwd_stats_f64: {name} has {t.numel()} elements, z {c} channels")
    out = _new_f64((7, c), z)
    _check(lib().vatl_bn_train_fwd_stats_f64(_f64(z), m, c, _f64(gamma), _f64(beta), _f64(running_mean), _f64(running_var), float(momentum), float(eps),
                                             _f64(out), _f64(_bn_ws(m, c, z.device, "f64")), _stream()), "vatl_bn_train_fwd_stats_f64")
    return out


def bn_apply_f64(z, scale, bias, residual, relu: bool):
    c = z.shape[-1]
    if scale.numel() != c or bias.numel() != c or (residual is not None and residual.shape != z.shape):
        raise VatlError(f"bn_apply_f64: scale / bias / residual do not match z {tuple(z.shape)}")
    y = torch.empty_like(z)
    _check(lib().vatl_bn_apply_f64(_f64(z), _f64(scale), _f64(bias), _f64(residual), _f64(y), z.numel() // c, c, int(relu), _stream()), "vatl_bn_apply_f64")
    return y


def bn_train_bwd_f64(dy, y, z, gamma, save_mean, save_invstd, want_g: bool = False):
    """-> dz, g (or None), dgamma, dbeta, all float64; y None: no ReLU mask."""
    c = z.shape[-1]
    m = z.numel() // c
    if dy.shape != z.shape or (y is not None and y.shape != z.shape) or save_mean.numel() != c or save_invstd.numel() != c:
        raise VatlError(f"bn_train_bwd_f64: dy / y / statistics do not match z {tuple(z.shape)}")
    dz = torch.empty_like(z)
    g = torch.empty_like(z) if want_g else None
    dgamma, dbeta = _new_f64((c,), z), _new_f64((c,), z)
    _check(lib().vatl_bn_train_bwd_f64(_f64(dy), _f64(y), _f64(z), _f64(gamma), _f64(save_mean), _f64(save_invstd), _f64(dz), _f64(g), _f64(dgamma),
                                       _f64(dbeta), m, c, _f64(_bn_ws(m, c, z.device, "f64")), _stream()), "vatl_bn_train_bwd_f64")
    return dz, g, dgamma, dbeta


def maxpool3x3s2_bwd_f64(dpool, x):
    """Gradient of MaxPool2d(3,2,1)'s input x (N,H,W,C) from dpool: first maximum in scan order takes it (torch's tie rule)."""
    n, h, w, c = _maxpool_bwd_shapes("maxpool3x3s2_bwd_f64", dpool, x)
    dx = torch.empty_like(x)
    _check(lib().vatl_maxpool3x3s2_bwd_f64(_f64(dpool), _f64(x), _f64(dx), n, h, w, c, _stream()), "vatl_maxpool3x3s2_bwd_f64")
    return dx


def col_sum_f64(x2d):
    """(..., C) float64 -> (C,) column sums in one fixed order."""
    c = x2d.shape[-1]
    m = x2d.numel() // c
    out = _new_f64((c,), x2d)
    _check(lib().vatl_col_sum_f64(_f64(x2d), m, c, _f64(out), _f64(_bn_ws(m, c, x2d.device, "f64")), _stream()), "vatl_col_sum_f64")
    return out


# ----------------------------------------------------------------------------
# 16-bit inference route (csrc/conv_h16.hip, csrc/glue_h16.hip): NHWC float16 / bfloat16 tensors, channels in multiples of 8
# ----------------------------------------------------------------------------

H16_DTYPES = {torch.float16: 0, torch.bfloat16: 1}          # the `dtype` argument of every vatl_*_h16 entry point


def _h16_code(dtype) -> int:
    if dtype not in H16_DTYPES:
        raise VatlError(f"the 16-bit route serves torch.float16 and torch.bfloat16, got {dtype}")
    return H16_DTYPES[dtype]


def _new_like(shape, like, dtype=None):
    return torch.empty(shape, device=like.device, dtype=dtype or like.dtype)


def pack_conv_weight_h16(w: torch.Tensor, dtype) -> torch.Tensor:
    """(Cout,Cin,R,S) fp32 -> [Cout][R][S][Cin8] of ``dtype``, Cin8 = Cin rounded up to 8 with zeros."""
    code = _h16_code(dtype)
    cout, cin, r, s = w.shape
    out = _new_like((cout, r, s, (cin + 7) // 8 * 8), w, dtype)
    _check(lib().vatl_pack_conv_weight_h16(_ptr(w.contiguous()), _ptr(out, dtype), cout, cin, r, s, code, _stream()), "vatl_pack_conv_weight_h16")
    return out


def pack_deconv_weight_h16(w: torch.Tensor, dtype) -> torch.Tensor:
    """ConvTranspose2d(4,2,1) weight (Cin,Cout,4,4) fp32 -> four 2x2 phase filters [4][Cout][2][2][Cin8] of ``dtype``."""
    code = _h16_code(dtype)
    cin, cout, kh, kw = w.shape
    if (kh, kw) != (4, 4):
        raise VatlError(f"pack_deconv_weight_h16: a 4x4 filter is needed, got {kh}x{kw}")
    out = _new_like((4, cout, 2, 2, (cin + 7) // 8 * 8), w, dtype)
    _check(lib().vatl_pack_deconv4x4s2_weight_h16(_ptr(w.contiguous()), _ptr(out, dtype), cin, cout, code, _stream()), "vatl_pack_deconv4x4s2_weight_h16")
    return out


def conv2d_fwd_h16(x, w_packed, scale, bias, stride: int, pad: int, relu: bool, residual=None, out_f32_nchw: bool = False, out=None):
    """x (N,H,W,Cin) fp16 / bf16, w_packed from pack_conv_weight_h16 -> (N,Ho,Wo,Cout) of x's dtype, or fp32 (N,Cout,Ho,Wo).
    scale / bias fp32 or None; residual (N,Ho,Wo,Cout) of x's dtype."""
    t = x.dtype
    code = _h16_code(t)
    n, h, w, cin = x.shape
    cout, r, s, cin_w = w_packed.shape
    if cin_w != cin:
        raise VatlError(f"conv2d_fwd_h16: input has {cin} channels, the filter {cin_w}")
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    shape = (n, cout, ho, wo) if out_f32_nchw else (n, ho, wo, cout)
    odt = torch.float32 if out_f32_nchw else t
    if out is None:
        out = _new_like(shape, x, odt)
    elif tuple(out.shape) != shape:
        raise VatlError(f"conv2d_fwd_h16: out has shape {tuple(out.shape)}, expected {shape}")
    if residual is not None and tuple(residual.shape) != (n, ho, wo, cout):
        raise VatlError(f"conv2d_fwd_h16: residual has shape {tuple(residual.shape)}, expected {(n, ho, wo, cout)}")
    _check(lib().vatl_conv2d_fwd_h16(_ptr(x, t), _ptr(w_packed, t), _ptr(scale), _ptr(bias), _ptr(residual, t), _ptr(out, odt), n, h, w, cin, cout, r, s,
                                     stride, pad, int(relu), int(out_f32_nchw), code, _stream()), "vatl_conv2d_fwd_h16")
    return out


def deconv4x4s2_fwd_h16(x, w_packed, scale, bias, relu: bool):
    t = x.dtype
    code = _h16_code(t)
    n, h, w, cin = x.shape
    cout = w_packed.shape[1]
    if w_packed.shape[-1] != cin:
        raise VatlError(f"deconv4x4s2_fwd_h16: input has {cin} channels, the filter {w_packed.shape[-1]}")
    y = _new_like((n, 2 * h, 2 * w, cout), x)
    _check(lib().vatl_deconv4x4s2_fwd_h16(_ptr(x, t), _ptr(w_packed, t), _ptr(scale), _ptr(bias), _ptr(y, t), n, h, w, cin, cout, int(relu), code, _stream()),
           "vatl_deconv4x4s2_fwd_h16")
    return y


def nchw_to_nhwc_h16(x: torch.Tensor, dtype) -> torch.Tensor:
    """(N,C,H,W) fp32 -> (N,H,W,C8) of ``dtype``: rounded to nearest even, channels C .. C8-1 exact zeros."""
    code = _h16_code(dtype)
    n, c, h, w = x.shape
    y = _new_like((n, h, w, (c + 7) // 8 * 8), x, dtype)
    _check(lib().vatl_nchw_to_nhwc_h16(_ptr(x), _ptr(y, dtype), n, c, h, w, code, _stream()), "vatl_nchw_to_nhwc_h16")
    return y


def nhwc_to_nchw_h16(x: torch.Tensor) -> torch.Tensor:
    """(N,H,W,C) fp16 / bf16 -> (N,C,H,W) fp32 (exact)."""
    code = _h16_code(x.dtype)
    n, h, w, c = x.shape
    y = _new_like((n, c, h, w), x, torch.float32)
    _check(lib().vatl_nhwc_to_nchw_h16(_ptr(x, x.dtype), _ptr(y), n, c, h, w, code, _stream()), "vatl_nhwc_to_nchw_h16")
    return y


def maxpool3x3s2_fwd_h16(x):
    code = _h16_code(x.dtype)
    n, h, w, c = x.shape
    y = _new_like((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), x)
    _check(lib().vatl_maxpool3x3s2_fwd_h16(_ptr(x, x.dtype), _ptr(y, x.dtype), n, h, w, c, code, _stream()), "vatl_maxpool3x3s2_fwd_h16")
    return y


def gap_fwd_h16(x, out=None):
    """(N,H,W,C) fp16 / bf16 -> (N,C) fp32: pixels summed in fp32 in order."""
    code = _h16_code(x.dtype)
    n, h, w, c = x.shape
    if out is None:
        out = _new_like((n, c), x, torch.float32)
    elif tuple(out.shape) != (n, c):
        raise VatlError(f"gap_fwd_h16: out has shape {tuple(out.shape)}, expected {(n, c)}")
    _check(lib().vatl_gap_fwd_h16(_ptr(x, x.dtype), _ptr(out), n, h * w, c, code, _stream()), "vatl_gap_fwd_h16")
    return out


def pixelshuffle2_fwd_h16(x):
    code = _h16_code(x.dtype)
    n, h, w, c = x.shape
    y = _new_like((n, 2 * h, 2 * w, c // 4), x)
    _check(lib().vatl_pixelshuffle2_fwd_h16(_ptr(x, x.dtype), _ptr(y, x.dtype), n, h, w, c, code, _stream()), "vatl_pixelshuffle2_fwd_h16")
    return y


def se_scale_add_relu_h16(x, gate, residual):
    """y = relu(x * sigmoid(gate) + residual): x, residual (N,H,W,C) fp16 / bf16, gate (N,C) fp32."""
    code = _h16_code(x.dtype)
    n, h, w, c = x.shape
    if tuple(gate.shape) != (n, c) or residual.shape != x.shape:
        raise VatlError("se_scale_add_relu_h16: gate must be (N,C) and the residual shaped like x")
    y = torch.empty_like(x)
    _check(lib().vatl_se_scale_add_relu_h16(_ptr(x, x.dtype), _ptr(gate), _ptr(residual, x.dtype), _ptr(y, x.dtype), n, h * w, c, code, _stream()),
           "vatl_se_scale_add_relu_h16")
    return y


def fuse_upsample_add_h16(base, ups, relu: bool):
    """base (N,H,W,C); ups = [(z, shift)] with z (N,H>>shift,W>>shift,C), at most 3, added in fp32 in list order."""
    t = base.dtype
    code = _h16_code(t)
    n, h, w, c = base.shape
    if len(ups) > 3:
        raise VatlError("fuse_upsample_add_h16: at most three up-sampled sources")
    for z, sh in ups:
        if tuple(z.shape) != (n, h >> sh, w >> sh, c):
            raise VatlError(f"fuse_upsample_add_h16: source {tuple(z.shape)} does not match {tuple(base.shape)} >> {sh}")
    y = torch.empty_like(base)
    a = list(ups) + [(None, 0)] * (3 - len(ups))
    _check(lib().vatl_fuse_upsample_add_h16(_ptr(base, t), _ptr(a[0][0], t), a[0][1], _ptr(a[1][0], t), a[1][1], _ptr(a[2][0], t), a[2][1], _ptr(y, t),
                                            n, h, w, c, int(relu), code, _stream()), "vatl_fuse_upsample_add_h16")
    return y


# ----------------------------------------------------------------------------
# bf16 fine-tune step (csrc/wgrad_h16.hip, csrc/train_glue_h16.hip, the data-gradient launcher of csrc/conv_h16.hip)
# ----------------------------------------------------------------------------

def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def wgrad_h16_splits(m: int) -> int:
    return int(lib().vatl_wgrad_h16_splits(m))


def conv2d_wgrad_h16(x, dz, cout: int, cin: int, r: int, s: int, stride: int, pad: int, transposed: bool = False, out=None):
    """Weight gradient in fp32: (cout,cin,r,s) from x (N,H,W,Cin8) and dz (N,Ho,Wo,Cout8) of one 16-bit dtype; ``transposed``:
    ConvTranspose2d(4,2,1) with x its forward input and dz (N,2H,2W,Cout8) its output gradient -> (cin,cout,4,4)."""
    t = x.dtype
    code = _h16_code(t)
    (n, h, w), m, rows8, cols8, out = _wgrad_shapes("conv2d_wgrad_h16", x, dz, cout, cin, r, s, stride, pad, transposed, out, 8, torch.float32)
    cin8, cout8 = x.shape[-1], dz.shape[-1]
    floats = int(lib().vatl_conv2d_wgrad_h16_workspace_floats(rows8, cols8, r, s, m))
    ws = torch.empty(floats, device=x.device, dtype=torch.float32)
    _check(lib().vatl_conv2d_wgrad_h16(_ptr(x, t), _ptr(dz, t), _ptr(ws), floats, n, h, w, cin8, cout8, r, s, stride, pad, int(transposed), code, _stream()),
           "vatl_conv2d_wgrad_h16")
    _check(lib().vatl_wgrad_h16_reduce(_ptr(ws), _ptr(out), m, cout, cin, r, s, int(transposed), _stream()), "vatl_wgrad_h16_reduce")
    return out


def pack_conv_weight_dgrad_h16(w: torch.Tensor, stride: int, pad: int, dtype) -> torch.Tensor:
    """(Cout,Cin,R,S) fp32 -> the flat data-gradient filters of conv2d_dgrad_h16 (Cin8*R*S*Cout8 elements of ``dtype``)."""
    code = _h16_code(dtype)
    cout, cin, r, s = w.shape
    out = _new_like((_pad8(cin) * r * s * _pad8(cout),), w, dtype)
    _check(lib().vatl_pack_conv_weight_dgrad_h16(_ptr(w.contiguous()), _ptr(out, dtype), cout, cin, r, s, stride, pad, code, _stream()),
           "vatl_pack_conv_weight_dgrad_h16")
    return out


# VatlPackJobH16.kind (include/vatl_hip.h: vatl_pack_weights_h16_multi) = which per-tensor packer's bytes the job writes
PACK_H16_CONV = 0                   # pack_conv_weight_h16: src (Cout,Cin,R,S)
PACK_H16_DECONV = 1                 # pack_deconv_weight_h16: src (Cin,Cout,4,4)
PACK_H16_DGRAD = 2                  # pack_conv_weight_dgrad_h16: src (Cout,Cin,R,S), every phase of (stride, pad)
_PACK_H16_SLICE = 1024              # destination elements per block


class _PackJobH16(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("first_block", C.c_int64), ("kind", C.c_int32), ("Cout", C.c_int32), ("Cin", C.c_int32),
                ("R", C.c_int32), ("S", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int32)]


class PackPlanH16:
    """The 16-bit filter re-packs of one bf16 training step as ONE launch (vatl_pack_weights_h16_multi): ``PackPlan``'s life cycle for
    the packers of the 16-bit route.

    The first step under a plan packs per tensor (``pack_conv_weight_h16`` / ``pack_deconv_weight_h16`` / ``pack_conv_weight_dgrad_h16``)
    and RECORDS each call: source tensor, kind, geometry and the destination, which is then kept.  ``seal()`` uploads the table.  From
    the next step on ``begin()`` refreshes every kept destination with one launch and ``lookup`` hands the kept buffers out — only while
    the source is the recorded storage at the version it had at ``begin()``; anything else makes the caller pack on the spot and the
    plan record again, into fresh buffers, at its next ``begin()``.

    The kept buffers are overwritten in place, so ``begin()`` has to come after the last reader of the previous step: it does on the
    same stream, and it makes the current stream wait for every other stream a step has been noted on since (``note_stream``)."""

    def __init__(self, dtype):
        self.dtype, self.code = dtype, _h16_code(dtype)
        self.jobs = {}            # key -> [src tensor, dst tensor, (kind, Cout, Cin, R, S, stride, pad), version at begin()]
        self.table = None
        self.total_blocks = 0
        self.ready = False
        self.stale = False
        self.streams = []         # where the kept buffers may still be read

    def note_stream(self):
        """The pass that starts now reads the kept buffers on the current stream."""
        cur = torch.cuda.current_stream()
        if cur not in self.streams:
            self.streams.append(cur)
        return cur

    def begin(self):
        cur = torch.cuda.current_stream()
        if self.ready and not self.stale:
            for st in self.streams:
                if st != cur:
                    cur.wait_stream(st)
            for j in self.jobs.values():
                j[3] = j[0]._version
            _check(lib().vatl_pack_weights_h16_multi(_ptr(self.table, torch.uint8), len(self.jobs), self.total_blocks, self.code, _stream()),
                   "vatl_pack_weights_h16_multi")
        else:
            for j in self.jobs.values():                     # let go of the kept buffers only behind their readers on other streams
                for st in self.streams:
                    if st != cur:
                        j[1].record_stream(st)
            self.jobs, self.table, self.total_blocks, self.ready, self.stale = {}, None, 0, False, False
        self.streams = [cur]

    def lookup(self, key, w):
        if not self.ready:
            return None
        j = self.jobs.get(key)
        if j is None or j[0].data_ptr() != w.data_ptr() or j[3] != w._version:
            self.stale = True                      # a filter the recording did not see, or weights that changed since begin()
            return None
        return j[1]

    @staticmethod
    def elements(kind: int, shape) -> int:
        """Destination elements of a job of ``kind`` whose source has ``shape``."""
        a, b, r, s = (int(v) for v in shape)
        if kind == PACK_H16_CONV:
            return a * r * s * _pad8(b)
        if kind == PACK_H16_DECONV:
            return 16 * b * _pad8(a)
        if kind == PACK_H16_DGRAD:
            return _pad8(b) * r * s * _pad8(a)
        raise VatlError(f"PackPlanH16: unknown kind {kind}")

    def record(self, key, w, dst, kind: int, stride: int = 1, pad: int = 0):
        """Note that ``dst`` holds the ``kind`` pack of ``w`` (just written by the per-tensor packer) and is to be kept."""
        if self.ready or key in self.jobs:
            return
        if w.dim() != 4 or w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous():
            raise VatlError("PackPlanH16: the source must be a contiguous 4-D fp32 device tensor")
        a, b, r, s = (int(v) for v in w.shape)
        if kind == PACK_H16_DECONV:
            if (r, s) != (4, 4):
                raise VatlError(f"PackPlanH16: a 4x4 filter is needed, got {r}x{s}")
            cout, cin = b, a
        else:
            cout, cin = a, b
        if kind == PACK_H16_DGRAD and (r > 7 or s > 7 or stride not in (1, 2) or pad < 0):
            raise VatlError(f"PackPlanH16: no data-gradient pack for a {r}x{s} filter with stride {stride}, pad {pad}")
        if dst.dtype != self.dtype or dst.device != w.device or not dst.is_contiguous() or dst.numel() != self.elements(kind, w.shape):
            raise VatlError(f"PackPlanH16: destination of {dst.numel()} {dst.dtype} elements does not fit kind {kind} of a {tuple(w.shape)} filter")
        self.jobs[key] = [w, dst, (kind, cout, cin, r, s, int(stride), int(pad)), w._version]

    def seal(self):
        if self.ready or not self.jobs:
            return
        arr = (_PackJobH16 * len(self.jobs))()
        blocks = 0
        for k, (src, dst, f, _) in enumerate(self.jobs.values()):
            jb = arr[k]
            jb.src, jb.dst, jb.first_block = src.data_ptr(), dst.data_ptr(), blocks
            jb.kind, jb.Cout, jb.Cin, jb.R, jb.S, jb.stride, jb.pad = f
            blocks += (dst.numel() + _PACK_H16_SLICE - 1) // _PACK_H16_SLICE
        dev = next(iter(self.jobs.values()))[1].device
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.total_blocks = blocks
        self.ready = True


def conv2d_dgrad_h16(dz, w_dgrad, xshape, r: int, s: int, stride: int, pad: int, residual=None):
    """dx (N,H,W,Cin8) = data gradient of a (r x s, stride, pad) conv from dz (N,Ho,Wo,Cout8); ``residual`` shaped like dx is added."""
    t = dz.dtype
    code = _h16_code(t)
    n, h, w, cin8, cout8 = _dgrad_shapes("conv2d_dgrad_h16", dz, w_dgrad, xshape, r, s, stride, pad, residual)
    dx = _new_like((n, h, w, cin8), dz)
    _check(lib().vatl_conv2d_dgrad_h16(_ptr(dz, t), _ptr(w_dgrad, t), _ptr(residual, t), _ptr(dx, t), n, h, w, cin8, cout8, r, s, stride, pad, code, _stream()),
           "vatl_conv2d_dgrad_h16")
    return dx


def bn_train_fwd_stats_h16(z, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """z NHWC fp16 / bf16 -> save_mean, save_invstd, scale, bias (C,) fp32; running statistics updated in place (None: not)."""
    code = _h16_code(z.dtype)
    c = z.shape[-1]
    m = z.numel() // c
    outs = [torch.empty(c, device=z.device, dtype=torch.float32) for _ in range(4)]
    _check(lib().vatl_bn_train_fwd_stats_h16(_ptr(z, z.dtype), m, c, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), momentum, eps,
                                             _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(_bn_ws(m, c, z.device, "h16"), torch.float64), code,
                                             _stream()), "vatl_bn_train_fwd_stats_h16")
    return outs


def bn_apply_h16(z, scale, bias, residual, relu: bool):
    code = _h16_code(z.dtype)
    c = z.shape[-1]
    y = torch.empty_like(z)
    _check(lib().vatl_bn_apply_h16(_ptr(z, z.dtype), _ptr(scale), _ptr(bias), _ptr(residual, z.dtype), _ptr(y, z.dtype), z.numel() // c, c, int(relu), code,
                                   _stream()), "vatl_bn_apply_h16")
    return y


def bn_train_bwd_h16(dy, y, z, gamma, save_mean, save_invstd, want_g: bool = False, dgamma=None, dbeta=None):
    """-> dz, g (or None), dgamma, dbeta; dy, y (or None: no ReLU mask), z of one 16-bit dtype, the rest fp32."""
    t = z.dtype
    code = _h16_code(t)
    c = z.shape[-1]
    m = z.numel() // c
    dz, dgamma, dbeta, coef = _bn_bwd_outs(z, dgamma, dbeta)
    g = torch.empty_like(z) if want_g else None
    _check(lib().vatl_bn_train_bwd_h16(_ptr(dy, t), _ptr(y, t), _ptr(z, t), _ptr(gamma), _ptr(save_mean), _ptr(save_invstd), _ptr(dz, t), _ptr(g, t),
                                       _ptr(dgamma), _ptr(dbeta), m, c, _ptr(coef), _ptr(_bn_ws(m, c, z.device, "h16"), torch.float64), code, _stream()),
           "vatl_bn_train_bwd_h16")
    return dz, g, dgamma, dbeta


def maxpool3x3s2_bwd_h16(dpool, x):
    """Gradient of MaxPool2d(3,2,1)'s input x (N,H,W,C) from dpool: first maximum in scan order takes it (torch's tie rule)."""
    code = _h16_code(x.dtype)
    n, h, w, c = _maxpool_bwd_shapes("maxpool3x3s2_bwd_h16", dpool, x)
    dx = torch.empty_like(x)
    _check(lib().vatl_maxpool3x3s2_bwd_h16(_ptr(dpool, x.dtype), _ptr(x, x.dtype), _ptr(dx, x.dtype), n, h, w, c, code, _stream()), "vatl_maxpool3x3s2_bwd_h16")
    return dx
