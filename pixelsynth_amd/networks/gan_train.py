"""What the multiscale discriminator's training pass runs besides its 4 x 4 convolutions (the reference's
models/networks/discriminators.py:97-114 and compute_generator_loss, models/losses/gan_loss.py:191-218):

instance_norm_lrelu_train(x, eps, slope)   LeakyReLU(InstanceNorm2d(affine=False)(x)) of an NCHW activation, per (sample, channel) plane
feature_matching(maps, weight)             weight * sum_k L1Loss(fake half of map k, real half detached), maps (2P, C_k, H_k, W_k) of a
                                           batch of P fakes followed by P reals -> (1,)

Two routes each:

  "hip"    csrc/gan_train.hip (libpixelsynth_gan_train.so) as torch.autograd.Functions, once differentiable: fp64 sums on the device, a
           plane held in registers between its reduction and its elementwise phase (one read and one write forward; two reads and one
           write backward), all maps of the feature matching in one launch forward and one backward.  For CUDA fp32 dense NCHW tensors.
  "torch"  the torch formula, autograd's own backward -- F.instance_norm + F.leaky_relu, F.l1_loss per map as the reference writes it:
           CPU, fp64, other layouts -- and everything under discriminator_train("torch").

The switch: discriminator_train(...) in effect, else opt.discriminator_train, else PS_DISCRIMINATOR_TRAIN, else the default below.
"""
import ctypes

import torch
import torch.nn.functional as F

from .. import _lib
from .routing import Switch, gpu_f32

discriminator_train = Switch("discriminator_train", "PS_DISCRIMINATOR_TRAIN", ("hip", "torch"), "hip", __name__, "DISCRIMINATOR_TRAIN",
                             attr="discriminator_train")
DISCRIMINATOR_TRAIN = discriminator_train.from_env()   # "hip" (the Functions below, where takes() holds) | "torch" (torch autograd)
mode = discriminator_train.resolve      # the route in effect
MAX_MAPS = 16                            # PS_GAN_TRAIN_MAX_MAPS of include/pixelsynth_gan_train.h: maps per call of the library
_WS = _lib.Workspace()


def takes(x):
    """What the HIP route takes: a CUDA fp32 (B, C, H, W) tensor, dense NCHW, not empty, planes and plane size below 2^31"""
    return (gpu_f32(x, layout=torch.contiguous_format) and x.numel() > 0 and x.size(0) * x.size(1) < 2 ** 31
            and x.size(2) * x.size(3) < 2 ** 31)


def norm_formula(x, eps=1e-5, slope=0.2):
    """The torch route"""
    return F.leaky_relu(F.instance_norm(x, eps=eps), slope)


class _InLrelu(torch.autograd.Function):
    """x (B, C, H, W) dense NCHW fp32.  Saves x, mean and rstd (one each per plane); v and the LeakyReLU's branch are recomputed."""

    @staticmethod
    def forward(ctx, x, eps, slope):
        planes, hw = x.size(0) * x.size(1), x.size(2) * x.size(3)
        y = torch.empty_like(x)
        mean, rstd = (torch.empty(planes, dtype=torch.float32, device=x.device) for _ in range(2))
        _lib.call("ps_in_lrelu_forward_f32", x, planes, hw, float(eps), float(slope), y, mean, rstd, None, 0)
        ctx.save_for_backward(x, mean, rstd)
        ctx.slope = float(slope)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, mean, rstd = ctx.saved_tensors
        dy = grad_y.to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        _lib.call("ps_in_lrelu_backward_f32", x, dy, mean, rstd, x.size(0) * x.size(1), x.size(2) * x.size(3), ctx.slope, dx, None, 0)
        return dx, None, None


def instance_norm_lrelu_train(x, eps=1e-5, slope=0.2, opt=None):
    """LeakyReLU(slope) of the instance normalisation (no affine, biased variance, eps) of x (B, C, H, W); differentiable once in x, works
    under torch.no_grad() too.  Module docstring: the routes."""
    if mode(opt) == "hip" and takes(x):
        return _InLrelu.apply(x, eps, slope)
    return norm_formula(x, eps, slope)


def feat_formula(maps, weight):
    """The torch route, as the reference adds it up: a (1,) accumulator, + L1Loss(fake, real.detach()) * weight per map in order"""
    total = torch.zeros(1, dtype=maps[0].dtype, device=maps[0].device)
    for m in maps:
        half = m.size(0) // 2
        total = total + F.l1_loss(m[:half], m[half:].detach()) * weight
    return total


def _tables(maps, weight):
    """The host tables of a call: map pointers, values per half, weights"""
    n = len(maps)
    return ((ctypes.c_void_p * n)(*[m.data_ptr() for m in maps]), (ctypes.c_longlong * n)(*[m.numel() // 2 for m in maps]),
            (ctypes.c_double * n)(*[float(weight)] * n))


class _FeatL1(torch.autograd.Function):
    """Up to MAX_MAPS dense fp32 maps on one device -> (1,) total; saves the maps (the sign of f - r is recomputed)"""

    @staticmethod
    def forward(ctx, weight, *maps):
        dev, n = maps[0].device, len(maps)
        ptrs, halves, weights = _tables(maps, weight)
        ws = _WS.query(dev, "ps_gan_feat_workspace_bytes", halves, n)
        per_map, total = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
        _lib.call("ps_gan_feat_l1_f32", ptrs, halves, weights, n, per_map, total, ws, ws.numel())
        ctx.save_for_backward(*maps)
        ctx.weight = float(weight)
        ctx.mark_non_differentiable(per_map)
        return total, per_map

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_total, _grad_per_map):
        maps = ctx.saved_tensors
        ptrs, halves, weights = _tables(maps, ctx.weight)
        grads = [torch.empty_like(m) for m in maps]
        gptrs = (ctypes.c_void_p * len(maps))(*[g.data_ptr() for g in grads])
        gt = grad_total.to(torch.float32).contiguous()
        _lib.call("ps_gan_feat_l1_backward_f32", ptrs, halves, weights, len(maps), gt, gptrs)
        return (None, *grads)


def feat_takes(m):
    """A map the HIP route takes: CUDA fp32, dense in its own order of dimensions, an even and positive number of samples"""
    return gpu_f32(m, layout=torch.contiguous_format, dims=None) and m.dim() >= 1 and m.size(0) % 2 == 0 and m.numel() > 0


def feature_matching(maps, weight, opt=None, per_map=False):
    """weight * sum over the maps of mean |fake half - real half|, -> (1,), with a gradient to the fake halves only (the real halves are
    detached, as in the reference).  More than MAX_MAPS maps: several calls of the library, their totals added in order.  per_map: also
    the unweighted means, (len(maps)), without a gradient."""
    maps = list(maps)
    if not maps:
        raise ValueError("feature_matching: no maps")
    if mode(opt) == "hip" and all(feat_takes(m) for m in maps) and len({m.device for m in maps}) == 1:
        total, parts = None, []
        for i in range(0, len(maps), MAX_MAPS):
            t, p = _FeatL1.apply(weight, *maps[i:i + MAX_MAPS])
            total = t if total is None else total + t
            parts.append(p)
        return (total, torch.cat(parts)) if per_map else total
    total = feat_formula(maps, weight)
    if per_map:
        with torch.no_grad():
            return total, torch.stack([F.l1_loss(m[:m.size(0) // 2], m[m.size(0) // 2:]) for m in maps])
    return total
