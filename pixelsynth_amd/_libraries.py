"""The table of the native libraries: what build.py compiles and _lib.py loads.  No imports beyond os (build.py runs without torch).

libpixelsynth_hip.so ("hip") is the C ABI of include/pixelsynth_hip.h, pinned at version 2; what was added after the pin (PercSim,
the homography consistency score, the FID network's passes, the batched chained-scene step, the AR plan's orders on the device, the scoring of best-of-N candidates, their ranking per view of a batch, the likelihood of given codes, the backward pass of the locally masked convolution, the backward pass of the splat and of the reprojection, the training half of the VQ-VAE's quantiser, the backward pass of the split-fp16 3 x 3 convolution, the noise-conditioned batch norm in training mode, the 1 x 1 shortcut's weight gradient and the resampling adjoints of a decoder block, the passes between the convolutions of the VGG19 content loss, the backward passes of the decoder's thin first and last layers, the instance norm + LeakyReLU and the feature-matching L1 of the discriminator's training pass, the passes between the masked convolutions of the PixelCNN's training pass and its cross entropy's backward, the depth head and the decoder-input blend of the generator's training step, the discriminator's 4 x 4 convolutions with their backward pass, the spectral normalisation of a network's layers in training, the batch norm + leaky ReLU and the relu -> bilinear x2 of a skip join of the depth Unet in training, the passes that make the VQ-VAE's convolutions differentiable and the backward passes of its 3-channel ends) lives in a library of its own beside it,
with its own header and its own last-error function, so that the pinned set of exports never moves.  A further library is one more
entry here and one prototype table in _lib.py.
"""
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
NO_CONTRACT = ["-ffp-contract=off"]

# name: the short name library(name) takes; so: the file beside this module; units: (translation unit of csrc/, its flags);
# headers: the public headers of include/ that declare its exports; last_error: the export that returns the text of a failure
Library = namedtuple("Library", "name so units headers last_error")

LIBRARIES = (
    Library("hip", "libpixelsynth_hip.so",
            [("splat.hip", NO_CONTRACT), ("zbuffer.hip", NO_CONTRACT), ("lmconv.hip", NO_CONTRACT), ("lmconv_grid.hip", NO_CONTRACT),
             ("lmconv_plan.hip", NO_CONTRACT), ("lmconv_column.hip", NO_CONTRACT), ("lmconv_tp.hip", NO_CONTRACT), ("vq.hip", NO_CONTRACT), ("nets.hip", NO_CONTRACT),
             ("conv_f16x3.hip", NO_CONTRACT + ["-Wno-inline-asm"]), ("conv_thin.hip", NO_CONTRACT), ("conv1x1.hip", NO_CONTRACT),
             ("vq_ends.hip", NO_CONTRACT), ("metrics.hip", NO_CONTRACT), ("host_order.cpp", [])],
            ("pixelsynth_hip.h", "pixelsynth_hip_debug.h"), "ps_last_error"),
    Library("percsim", "libpixelsynth_percsim.so", [("percsim.hip", NO_CONTRACT)], ("pixelsynth_percsim.h",), "ps_percsim_last_error"),
    Library("consistency", "libpixelsynth_consistency.so", [("consistency.hip", NO_CONTRACT)], ("pixelsynth_consistency.h",),
            "ps_consistency_last_error"),
    Library("fid", "libpixelsynth_fid.so", [("fid.hip", NO_CONTRACT)], ("pixelsynth_fid.h",), "ps_fid_last_error"),
    Library("scene", "libpixelsynth_scene.so", [("scene.hip", NO_CONTRACT)], ("pixelsynth_scene.h",), "ps_scene_last_error"),
    Library("plan", "libpixelsynth_plan.so", [("ar_order.hip", NO_CONTRACT)], ("pixelsynth_plan.h",), "ps_plan_last_error"),
    Library("rank", "libpixelsynth_rank.so", [("rank.hip", NO_CONTRACT)], ("pixelsynth_rank.h",), "ps_rank_last_error"),
    Library("rank_groups", "libpixelsynth_rank_groups.so", [("rank_groups.hip", NO_CONTRACT)], ("pixelsynth_rank_groups.h",),
            "ps_rank_groups_last_error"),
    Library("nll", "libpixelsynth_nll.so", [("code_nll.hip", NO_CONTRACT)], ("pixelsynth_nll.h",), "ps_nll_last_error"),
    Library("lmconv_bwd", "libpixelsynth_lmconv_bwd.so", [("lmconv_bwd.hip", NO_CONTRACT)], ("pixelsynth_lmconv_bwd.h",),
            "ps_lmconv_bwd_last_error"),
    Library("splat_bwd", "libpixelsynth_splat_bwd.so", [("splat_bwd.hip", NO_CONTRACT)], ("pixelsynth_splat_bwd.h",),
            "ps_splat_bwd_last_error"),
    Library("vq_train", "libpixelsynth_vq_train.so", [("vq_train.hip", NO_CONTRACT)], ("pixelsynth_vq_train.h",), "ps_vq_train_last_error"),
    Library("conv_bwd", "libpixelsynth_conv_bwd.so", [("conv_bwd.hip", NO_CONTRACT)], ("pixelsynth_conv_bwd.h",), "ps_conv_bwd_last_error"),
    Library("norm_train", "libpixelsynth_norm_train.so", [("norm_train.hip", NO_CONTRACT)], ("pixelsynth_norm_train.h",),
            "ps_norm_train_last_error"),
    Library("block_train", "libpixelsynth_block_train.so", [("block_train.hip", NO_CONTRACT)], ("pixelsynth_block_train.h",),
            "ps_block_train_last_error"),
    Library("content", "libpixelsynth_content.so", [("content_loss.hip", NO_CONTRACT)], ("pixelsynth_content.h",), "ps_content_last_error"),
    Library("thin_train", "libpixelsynth_thin_train.so", [("thin_train.hip", NO_CONTRACT)], ("pixelsynth_thin_train.h",),
            "ps_thin_train_last_error"),
    Library("pixelcnn_train", "libpixelsynth_pixelcnn_train.so", [("pixelcnn_train.hip", NO_CONTRACT)], ("pixelsynth_pixelcnn_train.h",),
            "ps_pixelcnn_train_last_error"),
    Library("train_glue", "libpixelsynth_train_glue.so", [("train_glue.hip", NO_CONTRACT)], ("pixelsynth_train_glue.h",),
            "ps_train_glue_last_error"),
    Library("spectral_train", "libpixelsynth_spectral_train.so", [("spectral_train.hip", NO_CONTRACT)], ("pixelsynth_spectral_train.h",),
            "ps_spectral_train_last_error"),
    Library("vq_conv_train", "libpixelsynth_vq_conv_train.so", [("vq_conv_train.hip", NO_CONTRACT)], ("pixelsynth_vq_conv_train.h",),
            "ps_vq_conv_train_last_error"),
    Library("unet_train", "libpixelsynth_unet_train.so", [("unet_train.hip", NO_CONTRACT)], ("pixelsynth_unet_train.h",),
            "ps_unet_train_last_error"),
    Library("disc_conv", "libpixelsynth_disc_conv.so", [("disc_conv.hip", NO_CONTRACT)], ("pixelsynth_disc_conv.h",),
            "ps_disc_conv_last_error"),
    Library("gan_train", "libpixelsynth_gan_train.so", [("gan_train.hip", NO_CONTRACT)], ("pixelsynth_gan_train.h",),
            "ps_gan_train_last_error"),
)
MAIN = LIBRARIES[0]


def path(entry):
    """Where the library lies: beside this module; PS_HIP_LIB (tuning builds) overrides the main one alone"""
    return (entry is MAIN and os.environ.get("PS_HIP_LIB")) or os.path.join(HERE, entry.so)
