"""The elementwise half of the depth regressor (architectures.Unet) in training: csrc/unet_train.hip (libpixelsynth_unet_train.so) as two
torch.autograd.Functions, once differentiable.

bn_act_train(x, module, slope=None) -> y or (y, z)   training-mode nn.BatchNorm2d on the batch's statistics: y = x * scale - shift with
                     scale = rstd * weight, shift = mean * scale - bias, and z = leaky_relu(y, slope) written in the same pass where `slope`
                     is given (going down the Unet y is the skip tensor and z what the next convolution reads).  fp64 sums on the device,
                     rounded once; the module's running_mean / running_var / num_batches_tracked are updated in place by the finishing
                     kernel.  The backward pass receives dy and dz (either may be absent), forms g = dy + dz * leaky'(y) inside its two
                     passes with y recomputed from x, and saves x, mean, rstd, weight and bias -- nothing activation-sized beyond x.
relu_up2_cat(a, b=None) -> (B, Ca + Cb, 2 H, 2 W)    F.interpolate(F.relu(torch.cat((a, b), 1)), scale_factor=2, mode="bilinear") in one
                     pass that reads a and b where they lie; the backward pass is one gather per operand, masked by the operand's sign.
                     Saves a and b.

Each takes what its takes_* says and hands everything else to the expressions Unet.forward ran before: the CPU, fp64, eval mode, N = 1,
momentum=None, InstanceNorm2d.  The switch: unet_train(...) in effect, else PS_UNET_TRAIN, else "torch" (the Unet keeps no options).

Out of scope: the encoder's 4 x 4 stride-2 convolutions, dconv1..3, the leaky ReLU behind the norm-less conv1, use_3D, InstanceNorm2d and
standing-stats norms, statistics synchronised across ranks, double backward.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .routing import Switch, empty_nhwc, gpu_f32, grad_nhwc

# with unet_train("hip"): ... -- in grad mode or in train() a Unet's norms and skip joins go through the Functions below and its wide 3 x 3
# convolutions through conv_routes._unet_train_conv; "torch": Unet.forward runs the expressions it always ran.
unet_train = Switch("unet_train", "PS_UNET_TRAIN", ("hip", "torch"), "torch", __name__, "UNET_TRAIN")
UNET_TRAIN = unet_train.from_env()
mode = unet_train.resolve           # the route in effect
MAX_PARTS, PART_ROWS, MAX_C = 256, 256, 65536       # PS_UNET_TRAIN_* of include/pixelsynth_unet_train.h
THREADS, MAX_CW = 256, 64
_WS = _lib.Workspace()


def active(module, x):
    """Whether Unet.forward takes its "hip" body: the route, a CUDA fp32 input, and grad mode or train()"""
    return mode() == "hip" and x.is_cuda and x.dtype == torch.float32 and (torch.is_grad_enabled() or module.training)


def plan(N, C):
    """Host mirror of the library's plan for N rows of C channels: (rows per part, parts, channel quads of a workgroup, its row lanes,
    workgroups across the channels)"""
    rows = PART_ROWS * -(-(-(-N // PART_ROWS)) // MAX_PARTS)
    cw = min(C // 4, MAX_CW)
    return rows, -(-N // rows), cw, THREADS // cw, -(-(C // 4) // cw)


def workspace_bytes(N, C):
    """Host mirror of ps_unet_train_workspace_bytes: the slab of (parts, 2, C) doubles and 2 C floats, each rounded up to 256 bytes"""
    up = lambda n: (n + 255) // 256 * 256
    return up(plan(N, C)[1] * 2 * C * 8) + up(2 * C * 4)


def _vec(t, x):
    """Whether t is a per-channel vector the kernels take: fp32 (C), contiguous, 16-byte aligned, on x's device"""
    return (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == x.size(1) and t.is_contiguous()
            and t.device == x.device and t.data_ptr() % 16 == 0)


def takes_bn(x, module):
    """What bn_act_train runs on HIP: x CUDA fp32 channels-last with C a multiple of 4 at a 16-byte address, N = B H W >= 2; a plain
    nn.BatchNorm2d in train() with affine parameters, track_running_stats and a numeric momentum"""
    if not (type(module) is nn.BatchNorm2d and module.training and module.track_running_stats and module.affine
            and isinstance(module.momentum, (int, float)) and module.running_mean is not None):
        return False
    if not (gpu_f32(x, multiple=4, aligned=True) and x.size(1) <= MAX_C and 2 <= x.numel() // x.size(1) < 2 ** 31):
        return False
    tracked = module.num_batches_tracked
    return (all(_vec(t, x) for t in (module.weight, module.bias, module.running_mean, module.running_var))
            and tracked is not None and tracked.dtype == torch.int64 and tracked.device == x.device)


def takes_up(a, b=None):
    """What relu_up2_cat runs on HIP: CUDA fp32 channels-last operands of one (B, ., H, W) with channels multiples of 4, 16-byte aligned"""
    if not (gpu_f32(a, multiple=4, aligned=True) and a.numel() > 0 and a.size(1) <= MAX_C and max(a.size(2), a.size(3)) < 2 ** 30):
        return False
    if b is None:
        return a.numel() < 2 ** 37
    return (gpu_f32(b, multiple=4, aligned=True) and b.device == a.device and b.size(1) <= MAX_C and b.size(0) == a.size(0)
            and b.shape[2:] == a.shape[2:] and a.numel() + b.numel() < 2 ** 37)


class _BnAct(torch.autograd.Function):
    """x (B, C, H, W) channels-last fp32; weight, bias (C).  -> y, or (y, z) with a slope.  The running statistics move in the forward."""

    @staticmethod
    def forward(ctx, x, weight, bias, module, slope):
        B, C, H, W = x.shape
        N, dev = B * H * W, x.device
        ws = _WS.query(dev, "ps_unet_train_workspace_bytes", N, C)
        mean, var, rstd = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(3))
        w, b = weight.detach(), bias.detach()
        _lib.call("ps_bn_stats_f32", x, N, C, float(module.eps), float(module.momentum), module.running_mean, module.running_var,
                  module.num_batches_tracked, mean, var, rstd, ws, ws.numel())
        # (what torch's own in-place update does to the version counters: what is cached from these buffers must see it)
        torch.autograd.graph.increment_version([module.running_mean, module.running_var, module.num_batches_tracked])
        y = torch.empty_like(x)         # (preserves channels_last)
        z = None if slope is None else torch.empty_like(x)
        _lib.call("ps_bn_act_apply_f32", x, mean, rstd, w, b, N, C, 0.0 if slope is None else float(slope), y, z)
        ctx.save_for_backward(x, mean, rstd, weight, bias)
        ctx.slope = slope
        ctx.set_materialize_grads(False)
        return y if slope is None else (y, z)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_z=None):
        x, mean, rstd, weight, bias = ctx.saved_tensors
        if grad_y is None and grad_z is None:
            return None, None, None, None, None
        B, C, H, W = x.shape
        N, dev = B * H * W, x.device
        dy = None if grad_y is None else _aligned(grad_nhwc(grad_y))
        dz = None if grad_z is None else _aligned(grad_nhwc(grad_z))
        ws = _WS.query(dev, "ps_unet_train_workspace_bytes", N, C)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dweight, dbias = torch.empty_like(mean), torch.empty_like(mean)
        _lib.call("ps_bn_act_backward_f32", x, dy, dz, mean, rstd, weight.detach(), bias.detach(), N, C,
                  0.0 if ctx.slope is None else float(ctx.slope), dx, dweight, dbias, ws, ws.numel())
        return dx, dweight if ctx.needs_input_grad[1] else None, dbias if ctx.needs_input_grad[2] else None, None, None


def _aligned(t):
    """t, or a copy of it where it does not start at a multiple of 16 bytes (a slice of a larger gradient)"""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format)


def bn_act_train(x, module, slope=None):
    """module(x) -- and, with `slope`, (module(x), F.leaky_relu(module(x), slope)) -- through csrc/unet_train.hip under unet_train("hip")
    where takes_bn(x, module) holds; anything else is module(x) and F.leaky_relu as torch runs them."""
    if mode() == "hip" and takes_bn(x, module):
        return _BnAct.apply(x, module.weight, module.bias, module, slope)
    y = module(x)
    return y if slope is None else (y, F.leaky_relu(y, slope))


class _ReluUp2Cat(torch.autograd.Function):
    """a (B, Ca, H, W), b (B, Cb, H, W) or None, channels-last fp32 -> (B, Ca + Cb, 2 H, 2 W) channels-last.  Saves a and b."""

    @staticmethod
    def forward(ctx, a, b):
        B, Ca, H, W = a.shape
        Cb = 0 if b is None else b.size(1)
        out = empty_nhwc(B, Ca + Cb, 2 * H, 2 * W, a)
        _lib.call("ps_relu_up2_cat_f32", a, b, B, H, W, Ca, Cb, out)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        a, b = ctx.saved_tensors
        B, Ca, H, W = a.shape
        C = Ca + (0 if b is None else b.size(1))
        g = _aligned(grad_nhwc(grad_out))
        grads, c0 = [], 0
        for k, src in enumerate((a, b)):
            if src is None or not ctx.needs_input_grad[k]:
                grads.append(None)
            else:
                d = torch.empty_like(src)
                _lib.call("ps_relu_up2_cat_backward_f32", g, src, B, H, W, C, c0, src.size(1), d)
                grads.append(d)
            c0 += 0 if src is None else src.size(1)
        return tuple(grads)


def relu_up2_cat(a, b=None):
    """bilinear x2 (align_corners=False) of relu(cat((a, b), 1)) through csrc/unet_train.hip under unet_train("hip") where takes_up(a, b)
    holds; anything else through the expressions Unet.forward ran before: relu, the 1 x 1 map's expand on the GPU, F.interpolate."""
    if mode() == "hip" and takes_up(a, b):
        return _ReluUp2Cat.apply(a, b)
    h = a if b is None else torch.cat((a, b), 1)
    if h.size(2) == 1 and h.size(3) == 1 and h.is_cuda:
        return F.relu(h).expand(-1, -1, 2, 2).contiguous(memory_format=torch.channels_last)
    return F.interpolate(F.relu(h), scale_factor=2, mode="bilinear", align_corners=False)
