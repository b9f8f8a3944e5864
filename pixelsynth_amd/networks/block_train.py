"""What a decoder block trains through between its 3 x 3 convolutions (f16x3.conv3x3_train) and its norms (norm_train.batch_norm_train):
the 1 x 1 projection on the other branch and the resample-and-sum that joins the two (csrc/block_train.hip,
libpixelsynth_block_train.so).  Both are torch.autograd.Functions, once differentiable, whose forward passes are the no-grad kernels
(csrc/conv1x1.hip, csrc/nets.hip) bit for bit.

conv1x1_train(x, weight, bias)     y = conv2d(x, weight, bias) for a 1 x 1 weight.  grad_input is the same 1 x 1 kernel on grad_y with the
                                   weight transposed (a torch matmul for channel counts that kernel does not take), grad_weight and
                                   grad_bias one GEMM over the pixels on the fp32 matrix pipe with the bias sums from the same read.
resample_sum_train(kind, a, b)     resample(a) + resample(b) -- bilinear x2 for "Up", avg_pool2d(., 3, 2, 1) for "Down" --, b may be None.
                                   The sum is linear and symmetric, so ONE adjoint pass serves both operands; nothing is saved but the shape.

The switch, for the decoder's blocks (networks/architectures.py): decoder_block_train(...) in effect, else opt.decoder_block_train, else
PS_DECODER_BLOCK_TRAIN; the default "torch" leaves every call where it was.
"""
import torch

from .. import _lib
from .routing import Switch, empty_nhwc, gpu_f32, grad_nhwc

# with decoder_block_train("hip"): ... -- in grad mode a decoder block's 1 x 1 projection (Ci and Co multiples of 64, at most 256) and its
# resample-and-sum inside go through conv1x1_train / resample_sum_train; "torch": through torch autograd, whatever the options say.
decoder_block_train = Switch("decoder_block_train", "PS_DECODER_BLOCK_TRAIN", ("hip", "torch"), "torch", __name__, "DECODER_BLOCK_TRAIN",
                             attr="decoder_block_train")
DECODER_BLOCK_TRAIN = decoder_block_train.from_env()   # "torch" (the shortcut and the join through torch autograd) | "hip" (the Functions below)
mode = decoder_block_train.resolve                     # the route in effect for a block whose options are `opt`
_WS = _lib.Workspace()
MAX_CHANNELS = 256


# ---- the 1 x 1 convolution ---------------------------------------------------------------------------------------------------------------
def conv1x1_takes(Ci, Co, npix):
    """The sizes conv1x1_train takes: what csrc/conv1x1.hip runs forward (Ci of 32, 64, 128, 256 here) and the grad_weight GEMM
    accepts -- Ci and Co multiples of 16 up to 256, a multiple of 16 pixels"""
    return (Ci % 16 == 0 and Co % 16 == 0 and 0 < Ci <= MAX_CHANNELS and 0 < Co <= MAX_CHANNELS and npix > 0 and npix % 16 == 0
            and bool(_lib.call("ps_conv1x1_takes", Ci, Co)))


class _Conv1x1Train(torch.autograd.Function):
    """x and the weight are saved, nothing else activation-sized; only what needs_input_grad asks for is computed"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, Ci, H, W = x.shape
        Co = weight.size(0)
        w2 = weight.detach().reshape(Co, Ci).contiguous()
        y = empty_nhwc(B, Co, H, W, x)
        _lib.call("ps_conv1x1_ex_nhwc_f32", x, Ci, w2, None if bias is None else bias.detach().contiguous(), None, 0, B * H * W, Ci, Co, y)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co, dev, npix = weight.size(0), x.device, B * H * W
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g = grad_nhwc(grad_y)
        gx = gw = gb = None
        if need_x:
            w2 = weight.detach().reshape(Co, Ci)
            if _lib.call("ps_conv1x1_takes", Co, Ci):
                gx = torch.empty_like(x)                                                  # (preserves channels_last)
                _lib.call("ps_conv1x1_nhwc_f32", g, w2.t().contiguous(), npix, Co, Ci, gx)
            else:
                gx = torch.matmul(g.permute(0, 2, 3, 1), w2).permute(0, 3, 1, 2)
        if need_w or need_b:
            ws = _WS.query(dev, "ps_conv1x1_grad_weight_workspace_bytes", npix, Ci, Co)
            gw = torch.empty((Co, Ci), dtype=torch.float32, device=dev)
            gb = torch.empty(Co, dtype=torch.float32, device=dev) if need_b else None
            _lib.call("ps_conv1x1_grad_weight_f32", x, g, npix, Ci, Co, gw, gb, ws, ws.numel())
            gw = gw.view(weight.shape) if need_w else None
        return gx, gw, gb


def conv1x1_train(x, weight, bias=None):
    """conv2d(x, weight, bias) for a 1 x 1 weight (stride 1, no padding) through csrc/conv1x1.hip, differentiable once in x, weight and
    bias.  x (B, Ci, H, W) channels_last fp32 on the device, weight (Co, Ci, 1, 1) or (Co, Ci), bias (Co) or None; conv1x1_takes(Ci, Co,
    B H W) sizes.  ValueError for anything else: the caller goes through torch."""
    if not (gpu_f32(x, aligned=True) and x.numel() > 0):
        raise ValueError("conv1x1_train: x must be a channels_last fp32 tensor (B, Ci, H, W) on the device")
    Ci = x.size(1)
    if not (weight.dim() in (2, 4) and weight.shape[:2] == (weight.size(0), Ci) and weight.numel() == weight.size(0) * Ci
            and weight.dtype == torch.float32 and weight.device == x.device
            and conv1x1_takes(Ci, weight.size(0), x.size(0) * x.size(2) * x.size(3))):
        raise ValueError(f"conv1x1_train: weight {tuple(weight.shape)} on x {tuple(x.shape)}: (Co, Ci[, 1, 1]) fp32 on x's device, Ci in "
                         "(32, 64, 128, 256), Co a multiple of 16 up to 256 and a multiple of 16 pixels required")
    if bias is not None and not (bias.shape == (weight.size(0),) and bias.dtype == torch.float32 and bias.device == x.device):
        raise ValueError("conv1x1_train: bias must be (Co) fp32 on x's device")
    return _Conv1x1Train.apply(x, weight, bias)


# ---- the join: resample both branches and add ----------------------------------------------------------------------------------------------
def resample_takes(kind, a, b=None):
    """What resample_sum_train takes: kind "Up" or "Down"; channels-last CUDA fp32 operands of equal shape with C a multiple of 4; even
    sides for "Down" """
    return (kind in ("Up", "Down") and gpu_f32(a, multiple=4, aligned=True) and a.numel() > 0
            and (b is None or (gpu_f32(b, aligned=True) and b.shape == a.shape and b.device == a.device))
            and (kind == "Up" or (a.size(2) % 2 == 0 and a.size(3) % 2 == 0)))


class _ResampleSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, a, b):
        B, C, H, W = a.shape
        if kind == "Up":
            out = empty_nhwc(B, C, 2 * H, 2 * W, a)
            _lib.call("ps_upsample_add_nhwc_f32", a, b, None, B, H, W, C, out)
        else:
            out = empty_nhwc(B, C, H // 2, W // 2, a)
            _lib.call("ps_pool_add_nhwc_f32", a, b, None, B, H, W, C, out)
        ctx.kind, ctx.shape, ctx.two = kind, tuple(a.shape), b is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        B, C, H, W = ctx.shape
        need_a, need_b = ctx.needs_input_grad[1], ctx.two and ctx.needs_input_grad[2]
        if not (need_a or need_b):
            return None, None, None
        g = grad_nhwc(grad_out)
        gin = empty_nhwc(B, C, H, W, g)
        _lib.call("ps_upsample_add_bwd_nhwc_f32" if ctx.kind == "Up" else "ps_pool_add_bwd_nhwc_f32", g, B, H, W, C, gin)
        return None, gin if need_a else None, gin if need_b else None


def resample_sum_train(kind, a, b=None):
    """resample(a) + resample(b) (b may be None: a alone) through csrc/nets.hip, differentiable once in a and b.  ValueError for what
    resample_takes refuses: the caller goes through torch."""
    if not resample_takes(kind, a, b):
        raise ValueError("resample_sum_train: kind 'Up' or 'Down' and channels_last fp32 operands of equal shape on the device required "
                         "(C a multiple of 4; even sides for 'Down')")
    return _ResampleSum.apply(kind, a, b)
