"""The noise-conditioned batch norm of the refinement decoder in training mode (the reference's bn.forward with manual_bn,
models/layers/normalization.py:114-200): batch statistics, the running or standing update of the stored ones, and gradients through both.

batch_norm_train(x, gain, bias, bn, relu, pend=None) -> y = [relu] (x * scale - shift), scale = rsqrt(var + eps) * gain,
shift = mean * scale - bias, with mean / var the biased statistics of x over (B, H, W).  Two routes:

  "hip"    csrc/norm_train.hip (libpixelsynth_norm_train.so) as a torch.autograd.Function, once differentiable: fp64 sums on the device
           (a variance the fp32 m2 - m^2 loses comes out right), two reads and a write forward, four reads and a write backward, the ReLU
           fused, its mask recomputed from x in the backward pass.  For what takes(x) says: CUDA fp32, channels-last storage, C % 4 == 0.
  "torch"  the formula in torch, autograd's own backward: CPU, fp64, NCHW, any C -- and everything under decoder_norm_train("torch").

The switch: decoder_norm_train(...) in effect, else PS_DECODER_NORM_TRAIN, else "hip" (nothing took this path before the routes existed).
Both routes update bn.stored_mean / bn.stored_var from detached statistics, under no_grad: the running average with bn.momentum, or, with
bn.accumulate_standing, sums and bn.accumulation_counter.  `pend` (C) is a convolution bias still missing from x: it shifts the batch mean
and nothing else, so it goes into the stored mean only -- y does not change, (x + pend) - (mean + pend) = x - mean.
"""
import torch

from .. import _lib
from .routing import Switch, gpu_f32, grad_nhwc, per_sample

# with decoder_norm_train("torch"): ... -- every training-mode noise-conditioned batch norm inside through the torch formula; "hip":
# through csrc/norm_train.hip where takes(x) holds.  The one switch without an option: the norm layers hold no `opt`.
decoder_norm_train = Switch("decoder_norm_train", "PS_DECODER_NORM_TRAIN", ("hip", "torch"), "hip", __name__, "DECODER_NORM_TRAIN")
DECODER_NORM_TRAIN = decoder_norm_train.from_env()
mode = decoder_norm_train.resolve      # the route in effect
_WS = _lib.Workspace()


def takes(x):
    """What the HIP route takes: a CUDA fp32 (B, C, H, W) tensor in channels-last storage with C a multiple of 4"""
    return gpu_f32(x, multiple=4) and x.numel() > 0


def _store(bn, mean, var, pend=None):
    """The stored statistics after a batch whose statistics are mean / var (C), as the reference updates them"""
    with torch.no_grad():
        mean, var = mean.detach().to(bn.stored_mean.dtype), var.detach().to(bn.stored_var.dtype)
        if pend is not None:
            mean = mean + pend.detach().to(mean.dtype)
        if bn.accumulate_standing:
            bn.stored_mean.copy_(bn.stored_mean + mean)
            bn.stored_var.copy_(bn.stored_var + var)
            bn.accumulation_counter += 1.0
        else:
            bn.stored_mean.copy_(bn.stored_mean * (1 - bn.momentum) + mean * bn.momentum)
            bn.stored_var.copy_(bn.stored_var * (1 - bn.momentum) + var * bn.momentum)


def batch_stats(x, bn, pend=None):
    """mean and biased variance of x over (B, H, W), each (1, C, 1, 1), the way the reference takes them (mean of squares minus squared
    mean, in fp32 for half inputs) -- differentiable; the stored statistics of `bn` move as a side effect."""
    xf = x.float() if x.dtype in (torch.float16, torch.bfloat16) else x
    m = xf.mean((0, 2, 3), keepdim=True)
    var = ((xf * xf).mean((0, 2, 3), keepdim=True) - m * m).to(x.dtype)
    m = m.to(x.dtype)
    _store(bn, m.reshape(-1), var.reshape(-1), pend)
    return m, var


def formula(x, gain, bias, bn, relu, pend=None):
    """The torch route: gain / bias broadcastable to (B, C, 1, 1)"""
    m, var = batch_stats(x, bn, pend)
    scale = torch.rsqrt(var + bn.eps) * gain
    y = x * scale - (m * scale - bias)
    return torch.relu(y) if relu else y


class _NormTrain(torch.autograd.Function):
    """x (B, C, H, W) channels-last fp32, gain / bias (B, C) contiguous on x's device.  Saves x, mean, rstd, gain and bias (the mask of
    the ReLU is recomputed from them); the stored statistics are updated by the statistics' finishing kernel."""

    @staticmethod
    def forward(ctx, x, gain, bias, bn, relu, pend):
        B, C, H, W = x.shape
        dev = x.device
        ws = _WS.query(dev, "ps_norm_train_workspace_bytes", B, H * W, C)
        mean, var, rstd = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(3))
        standing = bool(bn.accumulate_standing)
        keep, mom = (1.0, 1.0) if standing else (1.0 - bn.momentum, bn.momentum)
        _lib.call("ps_norm_train_stats_f32", x, pend, B, H * W, C, float(bn.eps), float(keep), float(mom), bn.stored_mean, bn.stored_var,
                  mean, var, rstd, ws, ws.numel())
        if standing:
            with torch.no_grad():
                bn.accumulation_counter += 1.0
        y = torch.empty_like(x)     # (preserves channels_last)
        _lib.call("ps_norm_train_apply_f32", x, mean, rstd, gain, bias, B, H * W, C, int(relu), y)
        ctx.save_for_backward(x, mean, rstd, gain, bias)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, mean, rstd, gain, bias = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        dy = grad_nhwc(grad_y)
        ws = _WS.query(dev, "ps_norm_train_workspace_bytes", B, H * W, C)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dgain, dbias = torch.empty_like(gain), torch.empty_like(gain)
        _lib.call("ps_norm_train_backward_f32", x, dy, mean, rstd, gain, bias, B, H * W, C, int(ctx.relu), dx, dgain, dbias, ws, ws.numel())
        return dx, dgain if ctx.needs_input_grad[1] else None, dbias if ctx.needs_input_grad[2] else None, None, None, None


def _plain(t, device):
    """t as the kernels take a per-channel vector or (B, C) table: fp32, contiguous, 16-byte aligned, on `device`"""
    return gpu_f32(t, layout=torch.contiguous_format, aligned=True, dims=None) and t.device == device


def batch_norm_train(x, gain, bias, bn, relu, pend=None):
    """[relu] of the batch norm of x (B, C, H, W) on its own statistics with the per-sample (or shared) gain and bias -- (B or 1, C),
    or anything that reshapes to it, such as (B, C, 1, 1) -- and the update of bn's stored statistics.  Differentiable once in x, gain
    and bias; works under torch.no_grad() too.  Module docstring: the routes and `pend`."""
    B, C = x.size(0), x.size(1)
    if (mode() == "hip" and takes(x) and _plain(bn.stored_mean, x.device) and _plain(bn.stored_var, x.device)
            and x.size(2) * x.size(3) * C < 2 ** 31 and gain.dtype == bias.dtype == torch.float32 and gain.device == bias.device == x.device
            and (pend is None or (pend.dtype == torch.float32 and pend.device == x.device and pend.numel() == C))):
        g2, b2 = per_sample(gain, B, C), per_sample(bias, B, C)
        if pend is not None:
            pend = pend.detach().reshape(C)
            if not _plain(pend, x.device):
                pend = pend.contiguous().clone()
        if x.data_ptr() % 16 == 0 and g2.data_ptr() % 16 == 0 and b2.data_ptr() % 16 == 0:
            return _NormTrain.apply(x, g2, b2, bn, relu, pend)
    shape = (-1, C, 1, 1)
    return formula(x, gain.reshape(shape), bias.reshape(shape), bn, relu, pend)
