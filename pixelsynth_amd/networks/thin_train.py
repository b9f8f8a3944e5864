"""The decoder's thin first and last layers in training mode: the convolutions that join a wide side of Cw channels (a multiple of 32, at
most 256) with a thin side (4 channels on the way in, 1 to 4 on the way out) -- block 0's 3 x 3 and 1 x 1 from 4 to 64 channels, block 7's
from 128 to 3 -- at the decoder's full resolution.  Two torch.autograd.Functions, once differentiable, that return conv(x) WITH its bias:

conv_thin_in_train(x, weight, bias)    4 -> Cw, k = 3 or 1.  Forward: the fp32 FMA kernel of csrc/conv_thin.hip (k = 3) or the 1 x 1 kernel of
                                       csrc/conv1x1.hip, bit for bit, then one rounded add of bias[co] (ps_thin_add_bias_f32 in place; the
                                       1 x 1 kernel adds it on its own way out).  grad_input: the thin-out / 1 x 1
                                       kernel on grad_y with the flipped, transposed weight.
conv_thin_out_train(x, weight, bias)   Cw -> T <= 4, k = 3 or 1.  Forward likewise on the thin-out / 1 x 1 kernel.  grad_input:
                                       ps_thin_expand_f32, one pass over the wide gradient.
grad_weight and grad_bias of both: ps_thin_grad_weight_f32, one read of the wide tensor (csrc/thin_train.hip, libpixelsynth_thin_train.so;
the orders of summation are in include/pixelsynth_thin_train.h).

The switch, for the decoder's blocks (conv_routes._conv_split): decoder_thin_train(...) in effect, else opt.decoder_thin_train, else
PS_DECODER_THIN_TRAIN; the default "torch" leaves every call where it was.
"""
import torch

from .. import _lib
from .routing import Switch, empty_nhwc, gpu_f32, grad_nhwc

# with decoder_thin_train("hip"): ... -- in grad mode a decoder block's thin 3 x 3 and 1 x 1 convolutions (takes_in / takes_out) go through
# the Functions below; "torch": through torch autograd, whatever the options say.
decoder_thin_train = Switch("decoder_thin_train", "PS_DECODER_THIN_TRAIN", ("hip", "torch"), "torch", __name__, "DECODER_THIN_TRAIN",
                            attr="decoder_thin_train")
DECODER_THIN_TRAIN = decoder_thin_train.from_env()   # "torch" (the thin layers through torch autograd) | "hip" (the Functions below)
mode = decoder_thin_train.resolve                    # the route in effect for a block whose options are `opt`
_WS = _lib.Workspace()
MAX_WIDE, THIN_IN = 256, 4


def _common(wide, k, H, W, w_multiple):
    return k in (1, 3) and wide % 32 == 0 and 0 < wide <= MAX_WIDE and H > 0 and W > 0 and H % 8 == 0 and W % w_multiple == 0


def takes_in(Ci, Co, k, H, W):
    """The sizes conv_thin_in_train takes: what ps_conv3x3_thin_in_nhwc_f32 runs forward and ps_conv3x3_thin_out_nhwc_f32 backward -- 4
    channels in, Co a multiple of 32 up to 256, H a multiple of 8, W of 64 -- and for k = 1 what the 1 x 1 kernel takes both ways"""
    return (Ci == THIN_IN and _common(Co, k, H, W, 64)
            and (k == 3 or bool(_lib.call("ps_conv1x1_takes", Ci, Co) and _lib.call("ps_conv1x1_takes", Co, Ci))))


def takes_out(Ci, Co, k, H, W):
    """The sizes conv_thin_out_train takes: what ps_conv3x3_thin_out_nhwc_f32 runs -- Ci a multiple of 32 up to 256, 1 to 4 channels out,
    H a multiple of 8, W of 32 -- and for k = 1 what the 1 x 1 kernel takes"""
    return 1 <= Co <= 4 and _common(Ci, k, H, W, 32) and (k == 3 or bool(_lib.call("ps_conv1x1_takes", Ci, Co)))


def _forward(x, weight, bias, thin_in):
    """The no-grad kernel on x and one rounded add of the bias: on the 1 x 1 kernel's way out, after the 3 x 3 kernels in place"""
    B, Ci, H, W = x.shape
    Co, k = weight.size(0), weight.size(2)
    w = weight.detach()
    bias = None if bias is None else bias.detach().contiguous()
    y = empty_nhwc(B, Co, H, W, x)
    if k == 1 and (bias is None or bias.data_ptr() % 16 == 0):
        _lib.call("ps_conv1x1_ex_nhwc_f32", x, Ci, w.reshape(Co, Ci).contiguous(), bias, None, 0, B * H * W, Ci, Co, y)
        return y
    if k == 1:
        _lib.call("ps_conv1x1_nhwc_f32", x, w.reshape(Co, Ci).contiguous(), B * H * W, Ci, Co, y)
    elif thin_in:
        _lib.call("ps_conv3x3_thin_in_nhwc_f32", x, None, None, w.permute(2, 3, 1, 0).contiguous(), B, H, W, Co, y)      # [ky][kx][ci][co]
    else:
        _lib.call("ps_conv3x3_thin_out_nhwc_f32", x, None, None, w.permute(2, 3, 1, 0).contiguous(), B, H, W, Ci, Co, y)
    if bias is not None:
        _lib.call("ps_thin_add_bias_f32", y, bias, B * H * W, Co)
    return y


def _aligned(t):
    """t, or a copy of it where it does not start at a multiple of 16 bytes (a slice of a larger gradient)"""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format)


def _grad_weight(thin, wide, k, wide_is_g, need_b):
    """-> (grad_weight [k][k][T][Cw], grad_bias or None) of ps_thin_grad_weight_f32"""
    B, T, H, W = thin.shape
    Cw, dev = wide.size(1), wide.device
    ws = _WS.query(dev, "ps_thin_train_workspace_bytes", B, H, W, Cw, T, k)
    gw = torch.empty((k, k, T, Cw), dtype=torch.float32, device=dev)
    gb = torch.empty(Cw if wide_is_g else T, dtype=torch.float32, device=dev) if need_b else None
    _lib.call("ps_thin_grad_weight_f32", thin, wide, B, H, W, Cw, T, k, int(wide_is_g), gw, gb, ws, ws.numel())
    return gw, gb


class _ConvThinInTrain(torch.autograd.Function):
    """4 -> Cw.  x and the weight are saved, nothing else activation-sized; only what needs_input_grad asks for is computed"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _forward(x, weight, bias, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co, k = weight.size(0), weight.size(2)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g = _aligned(grad_nhwc(grad_y))
        gx = gw = gb = None
        if need_x:
            gx = torch.empty_like(x)                                                  # (preserves channels_last)
            w = weight.detach()
            if k == 1:
                _lib.call("ps_conv1x1_nhwc_f32", g, w.reshape(Co, Ci).t().contiguous(), B * H * W, Co, Ci, gx)
            else:   # gx[q][ci] = sum_t sum_co W[co][ci][8 - t] g[q + off(t)][co]: the thin-out kernel's [tap][its Ci = Co][its Co = Ci]
                _lib.call("ps_conv3x3_thin_out_nhwc_f32", g, None, None, w.flip(2, 3).permute(2, 3, 0, 1).contiguous(), B, H, W, Co, Ci, gx)
        if need_w or need_b:
            gw, gb = _grad_weight(x, g, k, True, need_b)
            gw = gw.permute(3, 2, 0, 1).contiguous() if need_w else None              # [ky][kx][ci][co] -> (Co, Ci, k, k)
        return gx, gw, gb


class _ConvThinOutTrain(torch.autograd.Function):
    """Cw -> T.  x and the weight are saved; only what needs_input_grad asks for is computed"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _forward(x, weight, bias, False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co, k = weight.size(0), weight.size(2)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g = _aligned(grad_nhwc(grad_y))
        gx = gw = gb = None
        if need_x:   # gx[q][c] = sum_t sum_j W[j][c][k k - 1 - t] g[q + off(t)][j]
            gx = torch.empty_like(x)
            _lib.call("ps_thin_expand_f32", g, weight.detach().flip(2, 3).permute(2, 3, 0, 1).contiguous(), B, H, W, Co, Ci, k, gx)
        if need_w or need_b:
            gw, gb = _grad_weight(g, x, k, False, need_b)
            gw = gw.permute(2, 3, 0, 1).contiguous() if need_w else None              # [ky][kx][j][c] -> (T, Cw, k, k)
        return gx, gw, gb


def _check(name, x, weight, bias, takes, sizes):
    if not (gpu_f32(x, aligned=True) and x.numel() > 0):
        raise ValueError(f"{name}: x must be a channels_last fp32 tensor (B, Ci, H, W) on the device")
    Ci, Co = x.size(1), weight.size(0) if weight.dim() == 4 else 0
    if not (weight.dim() == 4 and weight.size(1) == Ci and weight.size(2) == weight.size(3) and weight.dtype == torch.float32
            and weight.device == x.device and takes(Ci, Co, weight.size(2), x.size(2), x.size(3)) and x.numel() // Ci < 2 ** 31):
        raise ValueError(f"{name}: weight {tuple(weight.shape)} on x {tuple(x.shape)}: (Co, Ci, k, k) fp32 on x's device, k 1 or 3, {sizes}")
    if bias is not None and not (bias.shape == (Co,) and bias.dtype == torch.float32 and bias.device == x.device):
        raise ValueError(f"{name}: bias must be (Co) fp32 on x's device")


def conv_thin_in_train(x, weight, bias=None):
    """conv2d(x, weight, bias, padding=k // 2) for a 4 -> Co convolution, differentiable once in x, weight and bias.  x (B, 4, H, W)
    channels_last fp32 on the device, weight (Co, 4, k, k), bias (Co) or None; takes_in sizes.  ValueError for anything else: the caller goes
    through torch."""
    _check("conv_thin_in_train", x, weight, bias, takes_in, "Ci = 4, Co a multiple of 32 up to 256, H a multiple of 8 and W of 64 required")
    return _ConvThinInTrain.apply(x, weight, bias)


def conv_thin_out_train(x, weight, bias=None):
    """conv2d(x, weight, bias, padding=k // 2) for a Ci -> Co <= 4 convolution, differentiable once in x, weight and bias.  x (B, Ci, H, W)
    channels_last fp32 on the device, weight (Co, Ci, k, k), bias (Co) or None; takes_out sizes.  ValueError for anything else: the caller
    goes through torch."""
    _check("conv_thin_out_train", x, weight, bias, takes_out,
           "Ci a multiple of 32 up to 256 (k = 1: 32, 64, 128 or 256), 1 <= Co <= 4, H a multiple of 8 and W of 32 required")
    return _ConvThinOutTrain.apply(x, weight, bias)
