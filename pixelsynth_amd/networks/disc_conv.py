"""The 4 x 4 convolutions of the discriminator's training pass (networks/discriminators.py: the spectrally normalised model1..3) on the
fp16 matrix pipe: csrc/disc_conv.hip behind libpixelsynth_disc_conv.so, include/pixelsynth_disc_conv.h states the arithmetic.

conv4x4_train(x, weight, stride, opt=None)   F.conv2d(x, weight, None, stride, 2) of a (Co, Ci, 4, 4) weight as a torch.autograd.Function,
                                              once differentiable in x and weight; x (B, Ci, H, W) dense NCHW -> (B, Co, Ho, Wo) dense NCHW,
                                              what gan_train.instance_norm_lrelu_train and gan_train.feature_matching take on their HIP routes

Every product is three fp16 MFMAs on split operands with fp32 sums.  The weight (weight_orig / sigma, entries around 1e-2) and grad_y are
multiplied by powers of two found, kept and applied on the device; nothing is read back and nothing synchronises, forward or backward; the
weight is packed by a kernel at every call (it moves every step).  Two runs give the same bits, grad_weight included; an element of the
output or of grad_input depends neither on its frame's place in the batch nor on the batch's size.  An x beyond fp16's range (|v| > 65000,
or not a number) raises f16x3.flag(device), a grad_y that is not finite f16x3.grad_flag(device) -- the conventions of f16x3._Conv3x3Train;
there is no check_weight (and no float(...)) on this route.

The switch: discriminator_conv_train("f16" | "torch") in effect, else opt.discriminator_conv_train, else PS_DISCRIMINATOR_CONV_TRAIN, else
"torch".  _SNConv.forward takes the "f16" route only with opt.isTrain, in grad mode and where takes() holds: everything else -- the
default, eval, the sample ranking, the CPU, ndf = 8, model0 and model4 -- is F.conv2d as before.  The switch is not one of
training.HIP_ROUTES; stack it: `with training.hip_routes(), discriminator_conv_train("f16"):`, or training.hip_routes_with_discriminator().
"""
import torch
import torch.nn.functional as F

from .. import _lib
from . import f16x3
from .routing import Switch, gpu_f32

discriminator_conv_train = Switch("discriminator_conv_train", "PS_DISCRIMINATOR_CONV_TRAIN", ("f16", "torch"), "torch", __name__,
                                  "DISCRIMINATOR_CONV_TRAIN", attr="discriminator_conv_train")
DISCRIMINATOR_CONV_TRAIN = discriminator_conv_train.from_env()   # "torch" (F.conv2d, autograd's backward) | "f16" (conv4x4_train)
mode = discriminator_conv_train.resolve
PAD = 2
_WS = _lib.Workspace()


def sizes_take(B, Ci, Co, H, W, stride, pad=PAD):
    """ps_disc_conv_takes of include/pixelsynth_disc_conv.h, mirrored (no library needed): stride 1 or 2, padding 2, Ci and Co multiples
    of 64 up to 512, H, W >= 1, every frame within 32-bit offsets"""
    if not (1 <= B <= 65535 and stride in (1, 2) and pad == 2 and H >= 1 and W >= 1 and 64 <= Ci <= 512 and 64 <= Co <= 512
            and Ci % 64 == 0 and Co % 64 == 0 and H < 2 ** 24 and W < 2 ** 24):
        return False
    Hp, Wp = H + 2 * pad, W + 2 * pad
    Ho, Wo = (Hp - 4) // stride + 1, (Wp - 4) // stride + 1
    Wo8 = -(-Wo // 8) * 8
    lim = 2 ** 31
    return (Hp * Wp * Ci < lim and (Ho + 2) * (Wo + 2) * Co < lim and Ci * Hp * Wo8 < lim and Co * Ho * Wo8 < lim
            and B * -(-(Ho * (Wo8 // 8)) // 2) < lim)


def operands_take(x, weight):
    """What the "f16" route asks of its tensors besides their device: x (B, Ci, H, W) fp32 dense NCHW and not empty, weight (Co, Ci, 4, 4)
    fp32 on x's device"""
    return (isinstance(x, torch.Tensor) and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0
            and isinstance(weight, torch.Tensor) and weight.dim() == 4 and weight.dtype == torch.float32 and weight.device == x.device
            and tuple(weight.shape[1:]) == (x.size(1), 4, 4))


def takes(x, weight, stride, pad=PAD):
    """What the "f16" route takes: CUDA tensors that operands_take, of sizes that sizes_take"""
    return (gpu_f32(x, layout=torch.contiguous_format) and operands_take(x, weight)
            and sizes_take(x.size(0), x.size(1), weight.size(0), x.size(2), x.size(3), stride, pad))


class _DiscConv(torch.autograd.Function):
    """x dense NCHW fp32, weight (Co, Ci, 4, 4).  Saves x and the weight (no packed copy: the backward pass packs again)."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        B, Ci, H, W = x.shape
        Co = weight.size(0)
        w = weight.detach().contiguous()
        sizes = (B, Ci, Co, H, W, stride, PAD)
        y = torch.empty((B, Co, (H + 2 * PAD - 4) // stride + 1, (W + 2 * PAD - 4) // stride + 1), dtype=torch.float32, device=x.device)
        ws = _WS.query(x.device, "ps_disc_conv_workspace_bytes", *sizes)
        _lib.call("ps_disc_conv_forward_f16x3", x, w, *sizes, y, f16x3.flag(x.device), ws, ws.numel())
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co, dev = weight.size(0), x.device
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_w):
            return None, None, None
        g = grad_y.to(torch.float32).contiguous()
        w = weight.detach().contiguous()
        sizes = (B, Ci, Co, H, W, ctx.stride, PAD)
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(w) if need_w else None
        scale2 = torch.empty(2, dtype=torch.float32, device=dev)
        ws = _WS.query(dev, "ps_disc_conv_workspace_bytes", *sizes)
        _lib.call("ps_disc_conv_backward_f16x3", x, w, g, *sizes, gx, gw, scale2, f16x3.flag(dev), f16x3.grad_flag(dev), ws, ws.numel())
        _DiscConv.last_scale2 = scale2       # (for the tests: the scale of the last backward pass, on the device)
        return gx, gw, None


def conv4x4_train(x, weight, stride, opt=None):
    """F.conv2d(x, weight, None, stride, 2) for a (Co, Ci, 4, 4) weight; through the kernels where takes() holds (whatever the switch
    says: the switch is _SNConv's), else through torch with autograd's own gradients.  `opt` is accepted for the callers' symmetry."""
    if takes(x, weight, stride):
        return _DiscConv.apply(x, weight, int(stride))
    return F.conv2d(x, weight, None, stride, PAD)
