"""ctypes binding of libpixelsynth_hip.so (the C ABI declared in include/pixelsynth_hip.h; the measurement / tuning / debugging
entry points tests, bench.py and tools use are declared in include/pixelsynth_hip_debug.h) and of the libraries beside it
(_libraries.LIBRARIES): one prototype table each, one loader, library(name).

The package calls the library through call() alone.  The product path has NO fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  Nothing here (or anywhere under pixelsynth_amd/) imports oracle/.
"""
import ctypes
import os

import numpy as np
import torch   # (before the library is loaded: see library())

from . import _libraries

LIB_PATH = _libraries.path(_libraries.MAIN)    # (PS_HIP_LIB: tuning builds)

c_void_p, c_int, c_float, c_double, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                                 ctypes.c_double, ctypes.c_size_t)
# Stand-ins of the table below.  RC as the restype: an int status, 0 = success (ps_last_error() says why not).  STREAM as the last
# parameter: the void *stream the call is queued on, which call() appends.  Both are declared to ctypes as c_int / c_void_p.
RC, STREAM = object(), object()

_PROTOS = {
    "ps_abi_version": (c_int, []),
    "ps_last_error": (ctypes.c_char_p, []),
    "ps_build_info": (ctypes.c_char_p, []),
    "ps_pixelcnn_launch_kinds": (c_int, []),
    "ps_pixelcnn_launch_kind_name": (ctypes.c_char_p, [c_int]),
    "ps_pixelcnn_launch_counts": (RC, [c_void_p, c_void_p, c_int]),
    "ps_pixelcnn_profile_begin": (RC, [c_void_p]),
    "ps_pixelcnn_profile_end": (RC, [c_void_p, c_int, c_void_p, c_void_p]),
    "ps_project_pts_f32": (RC, [c_void_p] * 5 + [c_int, c_int, c_void_p, STREAM]),
    "ps_project_pts_cumulative_f32": (RC, [c_void_p] * 8 + [c_int] * 4 + [c_void_p] * 2 + [STREAM]),
    "ps_splat_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_double]),
    "ps_splat_f32": (RC, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_int, c_float, c_int,
                          c_int, c_int] + [c_void_p] * 6 + [c_size_t, STREAM]),
    "ps_project_splat_f32": (RC, [c_void_p] * 6 + [c_int, c_int, c_int, c_double, c_int, c_float, c_int, c_int,
                                                   c_int, c_void_p, c_void_p, c_void_p, c_size_t, STREAM]),
    "ps_generation_order": (RC, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ps_ar_plan": (RC, [c_void_p, c_int, c_int, c_int] + [c_void_p] * 6),
    "ps_order_masks_f32": (RC, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, STREAM]),
    "ps_read_status": (RC, [c_void_p, STREAM]),
    "ps_custom_order": (RC, [c_int, c_int, c_void_p, c_void_p]),
    "ps_kernel_masks_f32": (RC, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "ps_lmconv_workspace_bytes": (c_size_t, [c_int] * 5),
    "ps_lmconv_forward_f32": (RC, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                   c_int, c_int, c_void_p, c_void_p, c_size_t, STREAM]),
    "ps_pixelcnn_create": (RC, [c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ps_pixelcnn_destroy": (None, [c_void_p]),
    "ps_pixelcnn_forward_f32": (RC, [c_void_p] * 5 + [c_int, c_void_p, STREAM]),
    "ps_pixelcnn_ar_run": (RC, [c_void_p] * 9 + [c_float, c_int, c_int, c_void_p, STREAM]),
    "ps_pixelcnn_ar_run_waves": (RC, [c_void_p] * 9 + [c_float, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, STREAM]),
    "ps_pixelcnn_ar_prefix": (RC, [c_void_p] * 7 + [c_int, c_int, c_int, c_int, STREAM]),
    "ps_pixelcnn_ar_prefix_frames": (RC, [c_void_p] * 7 + [c_int, c_void_p, c_int, c_int, c_int, c_int, STREAM]),
    "ps_pixelcnn_ar_columns": (RC, [c_void_p] * 9 + [c_float, c_int, c_int, c_void_p, c_void_p, c_int, STREAM]),
    "ps_pixelcnn_set_compute_units": (RC, [c_void_p, c_int]),
    "ps_stream_create_cu_range": (RC, [c_int, c_int, c_void_p]),
    "ps_stream_destroy": (RC, [STREAM]),     # (the stream to destroy: call it with stream=)
    "ps_pixelcnn_time_ar_run_waves": (RC, [c_void_p] * 8 + [c_float, c_int, c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 3 + [STREAM]),
    "ps_pixelcnn_time_ar_run_waves_range": (RC, [c_void_p] * 8 + [c_float, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int] + [c_void_p] * 3 + [STREAM]),
    "ps_ar_wavefronts": (RC, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ps_ar_wavefronts_capped": (RC, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ps_ar_wavefronts_frames": (RC, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "ps_pixelcnn_status": (RC, [c_void_p, STREAM]),
    "ps_pixelcnn_debug_cache": (c_void_p, [c_void_p, c_int, c_int]),
    "ps_pixelcnn_set_tuning": (RC, [c_void_p, ctypes.c_char_p, c_int]),
    "ps_pixelcnn_get_tuning": (RC, [c_void_p, ctypes.c_char_p, c_void_p]),
    "ps_zbuffer_scatter_f32": (RC, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 3 + [STREAM]),
    "ps_zbuffer_project_f32": (RC, [c_void_p] * 6 + [c_int, c_int] + [c_void_p] * 4 + [STREAM]),
    "ps_zbuffer_scatter_sorted_f32": (RC, [c_void_p] * 5 + [c_int] * 4 + [c_void_p] * 3 + [STREAM]),
    "ps_vq_nearest_f32": (RC, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, STREAM]),
    "ps_vq_embed_f32": (RC, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_affine_relu_nhwc_f32": (RC, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_pool_add_nhwc_f32": (RC, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_pool_add_post_nhwc_f32": (RC, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_upsample_add_nhwc_f32": (RC, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_add_bias_nhwc_f32": (RC, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_cat_mask_nhwc_f32": (RC, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_noise_affine_f32": (RC, [c_void_p] * 6 + [ctypes.c_float, c_int, c_int, c_int, c_void_p, c_void_p, STREAM]),
    "ps_conv3x3_thin_in_nhwc_f32": (RC, [c_void_p] * 4 + [c_int] * 4 + [c_void_p, STREAM]),
    "ps_conv3x3_thin_in_f16x3_nhwc": (RC, [c_void_p] * 4 + [c_int] * 4 + [c_void_p, c_void_p, STREAM]),
    "ps_conv3x3_thin_out_nhwc_f32": (RC, [c_void_p] * 4 + [c_int] * 5 + [c_void_p, STREAM]),
    "ps_vq_stem_s2d_f32": (RC, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_vq_head_f32": (RC, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_conv1x1_takes": (c_int, [c_int, c_int]),
    "ps_conv1x1_nhwc_f32": (RC, [c_void_p, c_void_p, ctypes.c_size_t, c_int, c_int, c_void_p, STREAM]),
    "ps_conv1x1_ex_nhwc_f32": (RC, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_size_t, c_int, c_int, c_void_p, STREAM]),
    "ps_conv3x3_f16x3_packed_bytes": (ctypes.c_size_t, [c_int, c_int]),
    "ps_conv3x3_f16x3_pack": (RC, [c_void_p, c_int, c_int, c_void_p, STREAM]),
    "ps_conv3x3_f16x3_nhwc": (RC, [c_void_p] * 6 + [c_int] * 5 + [c_void_p, c_void_p, STREAM]),
    "ps_conv3x3_f16x3_ex_nhwc": (RC, [c_void_p] * 6 + [c_int] * 8 + [c_void_p, c_void_p, STREAM]),
    "ps_pixelcnn_time_column_step": (RC, [c_void_p] * 6 + [c_int, c_int, c_int] + [c_void_p] * 4 + [STREAM]),
    "ps_pixelcnn_ar_step": (RC, [c_void_p] * 6 + [c_int, c_int, c_int, c_void_p, STREAM]),
    "ps_image_metrics_workspace_bytes": (c_size_t, [c_int] * 4),
    "ps_image_metrics": (RC, [c_void_p] * 4 + [c_int, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p, c_size_t, STREAM]),
}


# libpixelsynth_percsim.so (include/pixelsynth_percsim.h): the PercSim passes
PERCSIM_PROTOS = {
    "ps_percsim_last_error": (ctypes.c_char_p, []),
    "ps_percsim_workspace_bytes": (c_size_t, [c_int] * 3),
    "ps_percsim_input": (RC, [c_void_p] * 4 + [c_int, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p, STREAM]),
    "ps_percsim_tap": (RC, [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_size_t, STREAM]),
    "ps_percsim_finish": (RC, [c_void_p, c_size_t] + [c_int] * 3 + [c_void_p, c_void_p, STREAM]),
}

# libpixelsynth_consistency.so (include/pixelsynth_consistency.h): the homography consistency score
CONSISTENCY_PROTOS = {
    "ps_consistency_last_error": (ctypes.c_char_p, []),
    "ps_consistency_workspace_bytes": (c_size_t, [c_int] * 3),
    "ps_consistency": (RC, [c_void_p] * 4 + [c_int, c_void_p, c_void_p, c_int, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p, c_void_p,
                                                                                                         c_size_t, STREAM]),
}

# libpixelsynth_fid.so (include/pixelsynth_fid.h): the passes of the FID network
FID_PROTOS = {
    "ps_fid_last_error": (ctypes.c_char_p, []),
    "ps_fid_input": (RC, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, STREAM]),
    "ps_fid_conv_takes": (c_int, [c_int] * 7),
    "ps_fid_conv_co_tile": (c_int, [c_int]),
    "ps_fid_conv_packed_floats": (c_size_t, [c_int] * 4),
    "ps_fid_conv": (RC, [c_void_p, c_int, c_void_p, c_size_t, c_void_p] + [c_int] * 10 + [c_void_p, c_int, c_int, STREAM]),
    "ps_fid_pool": (RC, [c_void_p] + [c_int] * 6 + [c_void_p, c_int, c_int, STREAM]),
}

# libpixelsynth_scene.so (include/pixelsynth_scene.h): the batched chained-scene step over ragged clouds
SCENE_PROTOS = {
    "ps_scene_last_error": (ctypes.c_char_p, []),
    "ps_scene_state_bytes": (c_size_t, [c_int] * 3),
    "ps_scene_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_double]),
    "ps_scene_step_f32": (RC, [c_void_p] * 13 + [c_int] * 6 + [c_double, c_int, c_float, c_int, c_int, c_int, c_void_p, c_void_p,
                                                                c_void_p, c_size_t, STREAM]),
}

# libpixelsynth_plan.so (include/pixelsynth_plan.h): the generation orders of an AR plan from background masks on the device
PLAN_PROTOS = {
    "ps_plan_last_error": (ctypes.c_char_p, []),
    "ps_plan_order_takes": (c_int, [c_int, c_int]),
    "ps_plan_order": (RC, [c_void_p, c_int, c_int, c_int] + [c_void_p] * 4 + [STREAM]),
}

# libpixelsynth_rank.so (include/pixelsynth_rank.h): scoring and ranking the best-of-N candidates on the device
RANK_PROTOS = {
    "ps_rank_last_error": (ctypes.c_char_p, []),
    "ps_rank_classifier_input": (RC, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, STREAM]),
    "ps_rank_entropy": (RC, [c_void_p, c_int, c_int, c_void_p, STREAM]),
    "ps_rank_hinge_fake": (RC, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, STREAM]),
    "ps_rank_select": (RC, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, STREAM]),
}

# libpixelsynth_rank_groups.so (include/pixelsynth_rank_groups.h): the rank rule per view of a batch, and the winners' hand-over
c_long = ctypes.c_long
RANK_GROUPS_PROTOS = {
    "ps_rank_groups_last_error": (ctypes.c_char_p, []),
    "ps_rank_select_groups": (RC, [c_void_p, c_void_p, c_int, c_int, c_long, c_long, c_void_p, c_void_p, c_void_p, STREAM]),
    "ps_rank_take_groups": (RC, [c_void_p, c_void_p, c_int, c_int, c_long, c_long, c_long, c_void_p, STREAM]),
}

# libpixelsynth_nll.so (include/pixelsynth_nll.h): the likelihood of given codes under the PixelCNN's logits
NLL_PROTOS = {
    "ps_nll_last_error": (ctypes.c_char_p, []),
    "ps_code_nll_f32": (RC, [c_void_p, c_int, c_void_p, c_void_p, c_double, c_int, c_int] + [c_void_p] * 4 + [STREAM]),
}

# libpixelsynth_lmconv_bwd.so (include/pixelsynth_lmconv_bwd.h): the backward pass of the locally masked convolution
LMCONV_BWD_PROTOS = {
    "ps_lmconv_bwd_last_error": (ctypes.c_char_p, []),
    "ps_lmconv_bwd_workspace_bytes": (c_size_t, [c_int] * 5),
    "ps_lmconv_grad_weight_f32": (RC, [c_void_p, c_void_p, c_void_p, c_size_t] + [c_int] * 6 + [c_void_p, c_void_p, c_void_p, c_size_t, STREAM]),
    "ps_lmconv_adjoint_mask_f32": (RC, [c_void_p] + [c_int] * 4 + [c_void_p, STREAM]),
}

# libpixelsynth_splat_bwd.so (include/pixelsynth_splat_bwd.h): the backward pass of the soft z-buffer splat and of the reprojection
SPLAT_BWD_PROTOS = {
    "ps_splat_bwd_last_error": (ctypes.c_char_p, []),
    "ps_splat_bwd_workspace_bytes": (c_size_t, [c_int] * 3),
    "ps_splat_backward_f32": (RC, [c_void_p] * 5 + [c_int] * 4 + [c_double, c_int, c_float, c_int, c_int] + [c_void_p] * 3 + [c_size_t, STREAM]),
    "ps_project_pts_backward_f32": (RC, [c_void_p] * 6 + [c_int, c_int, c_void_p, STREAM]),
}

# libpixelsynth_vq_train.so (include/pixelsynth_vq_train.h): the training half of the VQ-VAE's quantiser
VQ_TRAIN_PROTOS = {
    "ps_vq_train_last_error": (ctypes.c_char_p, []),
    "ps_vq_train_workspace_bytes": (c_size_t, [c_int] * 3),
    "ps_vq_train_stats_f32": (RC, [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p] * 3 + [c_size_t, STREAM]),
    "ps_vq_train_quantize_f32": (RC, [c_void_p] * 3 + [c_int] * 3 + [c_void_p] * 3 + [c_size_t, STREAM]),
    "ps_vq_train_update_f32": (RC, [c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float] + [c_void_p] * 4 + [c_size_t, STREAM]),
    "ps_vq_train_backward_f32": (RC, [c_void_p] * 5 + [c_int] * 3 + [c_void_p, STREAM]),
}

# libpixelsynth_conv_bwd.so (include/pixelsynth_conv_bwd.h): the backward pass of the split-fp16 3 x 3 convolution
CONV_BWD_PROTOS = {
    "ps_conv_bwd_last_error": (ctypes.c_char_p, []),
    "ps_conv3x3_bwd_workspace_bytes": (c_size_t, [c_int] * 5),
    "ps_conv3x3_bwd_parts": (c_int, [c_int] * 5),
    "ps_conv3x3_bwd_prepare_f32": (RC, [c_void_p] + [c_int] * 4 + [c_void_p] * 4 + [c_size_t, STREAM]),
    "ps_conv3x3_grad_weight_f16x3": (RC, [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 3 + [c_size_t, STREAM]),
    "ps_conv3x3_bwd_unscale_f32": (RC, [c_void_p, c_size_t, c_void_p, STREAM]),
}

# libpixelsynth_norm_train.so (include/pixelsynth_norm_train.h): the noise-conditioned batch norm in training mode
NORM_TRAIN_PROTOS = {
    "ps_norm_train_last_error": (ctypes.c_char_p, []),
    "ps_norm_train_workspace_bytes": (c_size_t, [c_int] * 3),
    "ps_norm_train_parts": (c_int, [c_int] * 3),
    "ps_norm_train_stats_f32": (RC, [c_void_p, c_void_p] + [c_int] * 3 + [c_float] * 3 + [c_void_p] * 6 + [c_size_t, STREAM]),
    "ps_norm_train_apply_f32": (RC, [c_void_p] * 5 + [c_int] * 4 + [c_void_p, STREAM]),
    "ps_norm_train_backward_f32": (RC, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 4 + [c_size_t, STREAM]),
}

# libpixelsynth_block_train.so (include/pixelsynth_block_train.h): a decoder block's 1 x 1 weight gradient and resampling adjoints
BLOCK_TRAIN_PROTOS = {
    "ps_block_train_last_error": (ctypes.c_char_p, []),
    "ps_conv1x1_grad_weight_parts": (c_int, [c_size_t, c_int, c_int]),
    "ps_conv1x1_grad_weight_workspace_bytes": (c_size_t, [c_size_t, c_int, c_int]),
    "ps_conv1x1_grad_weight_f32": (RC, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, STREAM]),
    "ps_upsample_add_bwd_nhwc_f32": (RC, [c_void_p] + [c_int] * 4 + [c_void_p, STREAM]),
    "ps_pool_add_bwd_nhwc_f32": (RC, [c_void_p] + [c_int] * 4 + [c_void_p, STREAM]),
}

# libpixelsynth_content.so (include/pixelsynth_content.h): the passes between the convolutions of the VGG19 content loss
CONTENT_PROTOS = {
    "ps_content_last_error": (ctypes.c_char_p, []),
    "ps_content_tiles": (c_size_t, [c_size_t]),
    "ps_content_input": (RC, [c_void_p] * 4 + [c_int] * 3 + [c_void_p, STREAM]),
    "ps_content_bias": (RC, [c_void_p, c_void_p, c_size_t, c_int, STREAM]),
    "ps_content_tap": (RC, [c_void_p] + [c_int] * 4 + [c_void_p, STREAM]),
    "ps_content_finish": (RC, [c_void_p] * 5 + [STREAM]),
    "ps_content_pool": (RC, [c_void_p] + [c_int] * 4 + [c_void_p, STREAM]),
    "ps_content_join": (RC, [c_void_p] * 5 + [c_float] + [c_int] * 5 + [c_void_p, STREAM]),
}

# libpixelsynth_thin_train.so (include/pixelsynth_thin_train.h): the backward passes of the decoder's thin first and last layers
THIN_TRAIN_PROTOS = {
    "ps_thin_train_last_error": (ctypes.c_char_p, []),
    "ps_thin_train_parts": (c_int, [c_int] * 6),
    "ps_thin_train_workspace_bytes": (c_size_t, [c_int] * 6),
    "ps_thin_expand_f32": (RC, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, STREAM]),
    "ps_thin_grad_weight_f32": (RC, [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p] * 3 + [c_size_t, STREAM]),
    "ps_thin_add_bias_f32": (RC, [c_void_p, c_void_p, c_size_t, c_int, STREAM]),
}

# libpixelsynth_disc_conv.so (include/pixelsynth_disc_conv.h): the discriminator's 4 x 4 convolution on the fp16 matrix pipe, forward and backward
DISC_CONV_PROTOS = {
    "ps_disc_conv_last_error": (ctypes.c_char_p, []),
    "ps_disc_conv_takes": (c_int, [c_int] * 7),
    "ps_disc_conv_workspace_bytes": (c_size_t, [c_int] * 7),
    "ps_disc_conv_parts": (c_int, [c_int] * 7),
    "ps_disc_conv_forward_f16x3": (RC, [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p, c_void_p, c_void_p, c_size_t, STREAM]),
    "ps_disc_conv_backward_f16x3": (RC, [c_void_p] * 3 + [c_int] * 7 + [c_void_p] * 6 + [c_size_t, STREAM]),
}

# libpixelsynth_spectral_train.so (include/pixelsynth_spectral_train.h): the spectral normalisation of a table of layers in training,
# forward and backward.  The tables of ps_spectral_plan and grads are host arrays (ctypes arrays); table / table_host are host images
SPECTRAL_TRAIN_PROTOS = {
    "ps_spectral_train_last_error": (ctypes.c_char_p, []),
    "ps_spectral_table_bytes": (c_size_t, []),
    "ps_spectral_plan": (RC, [c_void_p] * 8 + [c_int, c_void_p, c_size_t] + [c_void_p] * 3),
    "ps_spectral_workspace_bytes": (c_size_t, [c_void_p]),
    "ps_spectral_forward_f32": (RC, [c_void_p] * 7 + [c_size_t, STREAM]),
    "ps_spectral_backward_f32": (RC, [c_void_p] * 9 + [c_size_t, STREAM]),
}

# libpixelsynth_unet_train.so (include/pixelsynth_unet_train.h): the depth Unet's batch norm + leaky ReLU and its relu -> bilinear x2 of a
# skip join, forward and backward
UNET_TRAIN_PROTOS = {
    "ps_unet_train_last_error": (ctypes.c_char_p, []),
    "ps_unet_train_workspace_bytes": (c_size_t, [c_int, c_int]),
    "ps_unet_train_parts": (c_int, [c_int, c_int]),
    "ps_bn_stats_f32": (RC, [c_void_p, c_int, c_int, c_float, c_float] + [c_void_p] * 7 + [c_size_t, STREAM]),
    "ps_bn_act_apply_f32": (RC, [c_void_p] * 5 + [c_int, c_int, c_float, c_void_p, c_void_p, STREAM]),
    "ps_bn_act_backward_f32": (RC, [c_void_p] * 7 + [c_int, c_int, c_float] + [c_void_p] * 4 + [c_size_t, STREAM]),
    "ps_relu_up2_cat_f32": (RC, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, STREAM]),
    "ps_relu_up2_cat_backward_f32": (RC, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, STREAM]),
}

# libpixelsynth_vq_conv_train.so (include/pixelsynth_vq_conv_train.h): the passes that make the VQ-VAE's convolutions differentiable (ReLU /
# space-to-depth pack, gate, fold) and the backward passes of its two 3-channel ends
VQ_CONV_TRAIN_PROTOS = {
    "ps_vq_conv_train_last_error": (ctypes.c_char_p, []),
    "ps_vq_conv_train_parts": (c_int, [ctypes.c_longlong]),
    "ps_vq_conv_train_workspace_bytes": (c_size_t, [ctypes.c_longlong]),
    "ps_vq_relu_pack_f32": (RC, [c_void_p] + [c_int] * 6 + [c_void_p, STREAM]),
    "ps_vq_gate_f32": (RC, [c_void_p] * 4 + [c_size_t, STREAM]),
    "ps_vq_fold_f32": (RC, [c_void_p] + [c_int] * 3 + [c_void_p, STREAM]),
    "ps_vq_ends_grad_weight_f32": (RC, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 3 + [c_size_t, STREAM]),
    "ps_vq_head_grad_input_f32": (RC, [c_void_p] * 3 + [c_int] * 3 + [c_void_p, STREAM]),
}

# libpixelsynth_gan_train.so (include/pixelsynth_gan_train.h): instance norm + LeakyReLU and the feature-matching L1 of the discriminator's
# training pass.  maps, half_elems, weights and grads are host tables (ctypes arrays)
GAN_TRAIN_PROTOS = {
    "ps_gan_train_last_error": (ctypes.c_char_p, []),
    "ps_in_lrelu_forward_f32": (RC, [c_void_p, c_int, c_int, c_float, c_float] + [c_void_p] * 4 + [c_size_t, STREAM]),
    "ps_in_lrelu_backward_f32": (RC, [c_void_p] * 4 + [c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, STREAM]),
    "ps_gan_feat_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "ps_gan_feat_l1_f32": (RC, [c_void_p] * 3 + [c_int] + [c_void_p] * 3 + [c_size_t, STREAM]),
    "ps_gan_feat_l1_backward_f32": (RC, [c_void_p] * 3 + [c_int, c_void_p, c_void_p, STREAM]),
}

# libpixelsynth_pixelcnn_train.so (include/pixelsynth_pixelcnn_train.h): PONO + skip + activation and the gate of the PixelCNN's gated
# blocks, forward and backward, and the backward pass of the cross entropy of given codes
PIXELCNN_TRAIN_PROTOS = {
    "ps_pixelcnn_train_last_error": (ctypes.c_char_p, []),
    "ps_pixelcnn_train_lanes": (c_int, [ctypes.c_longlong]),
    "ps_norm_act_forward_f32": (RC, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p] * 3 + [STREAM]),
    "ps_norm_act_backward_f32": (RC, [c_void_p, c_void_p, c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_void_p, c_void_p, STREAM]),
    "ps_gate_forward_f32": (RC, [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p] * 3 + [STREAM]),
    "ps_gate_backward_f32": (RC, [c_void_p] * 4 + [c_int] * 3 + [c_void_p, STREAM]),
    "ps_code_nll_backward_f32": (RC, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_double, c_int, c_int, c_void_p, c_void_p, STREAM]),
}

# libpixelsynth_train_glue.so (include/pixelsynth_train_glue.h): the depth head and the blend + mask channel into the decoder's NHWC input,
# forward and backward, of the generator's training step
TRAIN_GLUE_PROTOS = {
    "ps_train_glue_last_error": (ctypes.c_char_p, []),
    "ps_combine_mask_nhwc_f32": (RC, [c_void_p] * 3 + [c_int] * 3 + [c_void_p, STREAM]),
    "ps_combine_mask_nhwc_backward_f32": (RC, [c_void_p] * 2 + [c_int] * 3 + [c_void_p, STREAM]),
    "ps_depth_head_forward_f32": (RC, [c_void_p, c_int, c_double, c_double, ctypes.c_longlong, c_void_p, c_void_p, STREAM]),
    "ps_depth_head_backward_f32": (RC, [c_void_p, c_void_p, c_int, c_double, c_double, ctypes.c_longlong, c_void_p, STREAM]),
}

# short name of _libraries.LIBRARIES -> its prototype table; _OWNER: entry point -> the table entry of its library, built once
PROTOS = {"hip": _PROTOS, "percsim": PERCSIM_PROTOS, "consistency": CONSISTENCY_PROTOS, "fid": FID_PROTOS, "scene": SCENE_PROTOS,
          "plan": PLAN_PROTOS, "rank": RANK_PROTOS, "rank_groups": RANK_GROUPS_PROTOS, "nll": NLL_PROTOS, "lmconv_bwd": LMCONV_BWD_PROTOS, "splat_bwd": SPLAT_BWD_PROTOS,
          "vq_train": VQ_TRAIN_PROTOS, "conv_bwd": CONV_BWD_PROTOS, "norm_train": NORM_TRAIN_PROTOS,
          "block_train": BLOCK_TRAIN_PROTOS, "content": CONTENT_PROTOS, "thin_train": THIN_TRAIN_PROTOS,
          "pixelcnn_train": PIXELCNN_TRAIN_PROTOS, "train_glue": TRAIN_GLUE_PROTOS, "spectral_train": SPECTRAL_TRAIN_PROTOS,
          "vq_conv_train": VQ_CONV_TRAIN_PROTOS, "unet_train": UNET_TRAIN_PROTOS, "disc_conv": DISC_CONV_PROTOS, "gan_train": GAN_TRAIN_PROTOS}
_ENTRIES = {e.name: e for e in _libraries.LIBRARIES}
assert set(PROTOS) == set(_ENTRIES)
_OWNER = {fn: _ENTRIES[name] for name, table in PROTOS.items() for fn in table}
assert len(_OWNER) == sum(map(len, PROTOS.values())), "an entry point is declared in two prototype tables"
_loaded = {}


def exported_symbols():
    """Names every entry point include/pixelsynth_hip.h and include/pixelsynth_hip_debug.h declare (used by the CPU load test)."""
    return sorted(_PROTOS)


def library(name):
    """The loaded library `name` of _libraries.LIBRARIES, its prototypes declared to ctypes"""
    L = _loaded.get(name)
    if L is None:
        entry = _ENTRIES[name]
        main = entry is _libraries.MAIN
        if not main:
            lib()                      # the runtime binding below is the main library's: it loads first
        so = _libraries.path(entry)
        if not os.path.exists(so):
            raise RuntimeError(f"{so} is missing: build it with `python -m pixelsynth_amd.build` "
                               "(there is no CPU/PyTorch fallback for the HIP path)")
        # torch is imported first (top of this module): it brings its own libamdhip64/libhsa-runtime64, and this library has
        # to bind to THAT runtime instance (same streams, same allocations) instead of loading a second one.
        L = ctypes.CDLL(so)
        for fn_name, (res, args) in PROTOS[name].items():
            if main and not hasattr(L, fn_name):
                continue  # optional symbols (a tuning build's library) are checked by tests/test_abi.py
            fn = getattr(L, fn_name)
            fn.restype = c_int if res is RC else res
            fn.argtypes = [c_void_p if a is STREAM else a for a in args]
        _loaded[name] = L
    return L


def lib():
    return library("hip")


def check(rc, what):
    """Raise for a nonzero status of the entry point `what`, with its library's last error; any other label reports through
    libpixelsynth_hip.so's (callers name their calls freely)"""
    if rc != 0:
        entry = _OWNER.get(what, _libraries.MAIN)
        msg = getattr(library(entry.name), entry.last_error)()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


_BY_REF = (ctypes.Array, ctypes._SimpleCData)
_POINTERS = (c_void_p, ctypes.c_char_p, ctypes.c_wchar_p)


def call(name, *args, stream=None):
    """The entry point `name` (of any table of PROTOS; KeyError for a name none declares) on args: a torch tensor or numpy array goes
    as its data pointer, None as NULL, a ctypes scalar or array (an out-parameter, a small host table) by reference; anything else
    (ints, floats, bytes, the engine's handle) as ctypes converts it.  An entry point that ends in a STREAM gets the current stream
    appended (or `stream`), and each of its tensor arguments must be a CUDA tensor on the current device: else RuntimeError, before
    anything is queued.  A nonzero RC raises RuntimeError (check); any other return value is handed back."""
    owner = _OWNER[name].name
    res, types = PROTOS[owner][name]
    queued = bool(types) and types[-1] is STREAM
    if len(args) != len(types) - queued:
        raise TypeError(f"{name} takes {len(types) - queued} arguments{' besides the stream' if queued else ''}, got {len(args)}")
    fn = getattr(library(owner), name)
    conv, device = list(args), None
    for i, a in enumerate(args):
        if isinstance(a, torch.Tensor):
            if queued:
                if not a.is_cuda:
                    raise RuntimeError(f"{name}: args[{i}] is a CPU tensor; the pixelsynth_amd HIP path needs tensors on the ROCm "
                                       "device (there is no CPU fallback)")
                if device is None:
                    device = torch.cuda.current_device()
                if a.device.index != device:
                    raise RuntimeError(f"{name}: args[{i}] is on {a.device}, the call is queued on the current device cuda:{device}")
            conv[i] = a.data_ptr()
        elif isinstance(a, np.ndarray):
            conv[i] = a.ctypes.data
        elif isinstance(a, _BY_REF) and not isinstance(a, _POINTERS):
            conv[i] = ctypes.byref(a)
    if queued:
        conv.append(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    elif stream is not None:
        raise TypeError(f"{name} takes no stream")
    rc = fn(*conv)
    if res is RC:
        check(rc, name)
    return rc


class Workspace:
    """Scratch owned by PyTorch (the library never allocates); grown on demand, kept per device.  One instance per user whose sizes
    alternate, so that none regrows the other's."""

    def __init__(self):
        self.buf = {}

    def get(self, device, nbytes):
        t = self.buf.get(device)
        if t is None or t.numel() < nbytes:
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self.buf[device] = t
        return t

    def query(self, device, name, *sizes):
        """get() of what the entry point `name` asks for on `sizes`; an answer of 0 is its refusal of them"""
        n = call(name, *sizes)
        if n == 0:
            raise RuntimeError(f"{name}: invalid sizes")
        return self.get(device, n)


def ptr(t):
    """Device (or host) pointer of a contiguous torch tensor / numpy array, or None."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return ctypes.c_void_p(t.data_ptr())
    return ctypes.c_void_p(t.ctypes.data)


def current_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_STATUS = {}


def status_word(device=None):
    """The caller-owned status word (int32, zero) of a device that asynchronous entry points raise bits in
    (include/pixelsynth_hip.h: PS_STATUS_*); one per device, owned by this binding -- the library keeps none."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _STATUS.get(idx)
    if t is None:
        t = _STATUS[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return t


def read_status(what, device=None):
    """Synchronise the current stream OF THE STATUS WORD'S DEVICE and raise if an asynchronous call (`what`) raised a bit in it."""
    word = status_word(device)
    with torch.cuda.device(word.device):
        try:
            call("ps_read_status", word)
        except RuntimeError as err:
            raise RuntimeError(f"{what}: {err}") from None


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("pixelsynth_amd HIP path needs tensors on the ROCm device "
                               "(got a CPU tensor; there is no CPU fallback)")
