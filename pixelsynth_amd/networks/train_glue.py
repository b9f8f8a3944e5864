"""The full-resolution passes between the units of the generator's training step (ZbufferModelPts.forward_train; the reference's
models/z_buffermodel.py forward_image :303-311 and get_combined :703-708):

combine_mask_nhwc(gen_fs, input_gt, background_mask)   the blend gen_fs * fg + input_gt * bg, joined with the mask channel fg, as the
                                                       (B,4,H,W) channels-last tensor ResNetDecoder reads first
depth_head(raw, mode, min_z, max_z)                    the regressor's output -> (depth, PredDepthImg = depth / 5 - 1)

Two routes each:

  "hip"    csrc/train_glue.hip (libpixelsynth_train_glue.so) as torch.autograd.Functions, once differentiable: one launch forward and
           one backward per call, elementwise, so a frame's bits depend on neither the batch nor the launch.  combine_mask_nhwc saves
           the mask alone, depth_head `raw` alone (the sigmoid is recomputed).  For CUDA fp32 dense tensors: gen_fs and input_gt
           (B,3,H,W) NCHW with input_gt not requiring grad, a bool mask (B,H,W); raw (B,1,H,W).
  "torch"  the torch formula, autograd's own backward -- get_combined + cat, torch.sigmoid and the scaling, literally: the CPU, fp64,
           C != 3, an input_gt that requires grad, other storages -- and everything under train_glue("torch").

combine_mask_nhwc's two routes give the same bits, forward and backward: the arithmetic is the formula's (two products and one
addition per value, no contraction).  depth_head's differ by rounding (expf and a true division against torch's sigmoid kernel;
depth / 5 a true division where torch's device kernel multiplies by the rounded reciprocal): tests/_train_glue_ref.py derives the bound.

The switch: train_glue(...) in effect, else opt.train_glue, else PS_TRAIN_GLUE, else "hip" -- nothing took this path before.
"""
import torch

from .. import _lib
from .routing import Switch, gpu_f32

train_glue = Switch("train_glue", "PS_TRAIN_GLUE", ("hip", "torch"), "hip", __name__, "TRAIN_GLUE", attr="train_glue")
TRAIN_GLUE = train_glue.from_env()       # "hip" (the Functions below, where they take the tensors) | "torch" (the formulas)
mode = train_glue.resolve                # the route in effect

DEPTH_RANGE, DEPTH_INVERSE = 0, 1        # PS_GLUE_DEPTH_* of include/pixelsynth_train_glue.h


# ------------------------------------------------------------------------------------------------------------------ the torch route
def combine_mask_formula(gen_fs, input_gt, background_mask):
    """get_combined (z_buffermodel.py:703-708), then the decoder's torch.cat with the mask channel -> (B,C+1,H,W), channels-last on the GPU"""
    b, h, w = background_mask.shape
    fg = (~background_mask).float().to(gen_fs.dtype)
    bg = background_mask.float().to(gen_fs.dtype)
    combined = gen_fs * fg.view(b, -1, h, w) + input_gt * bg.view(b, -1, h, w)
    x = torch.cat((combined, fg.unsqueeze(1)), 1)
    return x.contiguous(memory_format=torch.channels_last) if x.is_cuda else x


def depth_head_formula(raw, mode_, min_z, max_z):
    """z_buffermodel.py:303-314 and the PredDepthImg of :388 -> (depth, PredDepthImg detached)"""
    s = torch.sigmoid(raw)
    depth = 1. / (s * 10 + 0.01) if mode_ == DEPTH_INVERSE else s * (max_z - min_z) + min_z
    return depth, (depth / 5 - 1).detach()


# -------------------------------------------------------------------------------------------------------------------- the HIP route
def combine_takes(gen_fs, input_gt, background_mask):
    """What ps_combine_mask_nhwc_f32 takes: see the module docstring"""
    return (gpu_f32(gen_fs, layout=torch.contiguous_format) and gpu_f32(input_gt, layout=torch.contiguous_format)
            and gen_fs.size(1) == 3 and gen_fs.numel() > 0 and input_gt.shape == gen_fs.shape and input_gt.device == gen_fs.device
            and not (torch.is_grad_enabled() and input_gt.requires_grad)
            and torch.is_tensor(background_mask) and background_mask.dtype == torch.bool and background_mask.is_contiguous()
            and background_mask.device == gen_fs.device
            and background_mask.shape == (gen_fs.size(0), gen_fs.size(2), gen_fs.size(3))
            and gen_fs.size(0) * gen_fs.size(2) * gen_fs.size(3) < 2 ** 31)


def depth_takes(raw):
    """What ps_depth_head_forward_f32 takes: CUDA fp32 (B,1,H,W), dense, not empty, fewer than 2^31 values"""
    return gpu_f32(raw, layout=torch.contiguous_format) and raw.size(1) == 1 and 0 < raw.numel() < 2 ** 31


def _aligned(t):
    """t, or a copy of it where it does not start at a multiple of 16 bytes (a view into a larger buffer)"""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format)


class CombineMaskNHWC(torch.autograd.Function):
    """gen_fs, input_gt (B,3,H,W) dense NCHW fp32, mask (B,H,W) bool -> (B,4,H,W) in (B,H,W,4) storage.  Saves the mask alone."""

    @staticmethod
    def forward(ctx, gen_fs, input_gt, background_mask):
        B, _, H, W = gen_fs.shape
        out = torch.empty((B, H, W, 4), dtype=torch.float32, device=gen_fs.device)
        with torch.cuda.device(gen_fs.device):
            _lib.call("ps_combine_mask_nhwc_f32", gen_fs, input_gt, background_mask, B, H, W, out)
        ctx.save_for_backward(background_mask)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (mask,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        B, H, W = mask.shape
        g = _aligned(grad_out.to(torch.float32).permute(0, 2, 3, 1).contiguous())
        grad_gen = torch.empty((B, 3, H, W), dtype=torch.float32, device=mask.device)
        with torch.cuda.device(mask.device):
            _lib.call("ps_combine_mask_nhwc_backward_f32", g, mask, B, H, W, grad_gen)
        return grad_gen, None, None


class DepthHead(torch.autograd.Function):
    """raw (B,1,H,W) dense fp32 -> (depth, PredDepthImg), the second marked non-differentiable.  Saves raw alone."""

    @staticmethod
    def forward(ctx, raw, mode_, min_z, max_z):
        depth, pred = torch.empty_like(raw), torch.empty_like(raw)
        with torch.cuda.device(raw.device):
            _lib.call("ps_depth_head_forward_f32", raw, mode_, min_z, max_z, raw.numel(), depth, pred)
        ctx.save_for_backward(raw)
        ctx.args = (mode_, min_z, max_z)
        ctx.mark_non_differentiable(pred)
        return depth, pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_depth, _grad_pred):
        (raw,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        g = grad_depth.to(torch.float32).contiguous()
        grad_raw = torch.empty_like(raw)
        mode_, min_z, max_z = ctx.args
        with torch.cuda.device(raw.device):
            _lib.call("ps_depth_head_backward_f32", raw, g, mode_, min_z, max_z, raw.numel(), grad_raw)
        return grad_raw, None, None, None


# ------------------------------------------------------------------------------------------------------------------ the front ends
def combine_mask_nhwc(gen_fs, input_gt, background_mask, opt=None):
    """The decoder's first input in one pass: get_combined(gen_fs, input_gt, background_mask) joined with the mask channel
    (~background_mask).float(), as a (B,4,H,W) tensor in channels-last storage -- hand it to ResNetDecoder WITHOUT the mask argument.
    Differentiable once, in gen_fs alone on the HIP route.  Module docstring: the routes."""
    if mode(opt) == "hip" and combine_takes(gen_fs, input_gt, background_mask):
        return CombineMaskNHWC.apply(gen_fs, input_gt, background_mask)
    return combine_mask_formula(gen_fs, input_gt, background_mask)


def depth_head(raw, mode_=DEPTH_RANGE, min_z=0.0, max_z=1.0, opt=None):
    """The reference's depth rule on the regressor's output `raw` (B,1,H,W): sigmoid scaled to [min_z, max_z] (mode 0) or
    1 / (10 sigmoid + 0.01) (mode 1, opt.use_inverse_depth) -> (depth, PredDepthImg = depth / 5 - 1, without gradient)"""
    if mode_ not in (DEPTH_RANGE, DEPTH_INVERSE):
        raise ValueError(f"depth_head: mode is {mode_!r}, expected 0 (range) or 1 (inverse)")
    if mode(opt) == "hip" and depth_takes(raw):
        return DepthHead.apply(raw, int(mode_), float(min_z), float(max_z))
    return depth_head_formula(raw, mode_, min_z, max_z)
