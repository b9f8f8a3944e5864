"""Locally masked convolution on MI355X -- drop-in for the reference's
models/lmconv/locally_masked_convolution.py: the forward (:11-50) and the custom backward (:52-93).

The reference builds im2col (F.unfold), multiplies by the per-location 3x3 mask and calls matmul
(:25-42).  Here one C-ABI call (ps_lmconv_forward_f32 -> csrc/lmconv.hip:k_gemm) gathers the masked
taps straight from a channels-last copy of x into v_mfma_f32_16x16x4_f32 tiles.  The backward is HIP as well
(csrc/lmconv_bwd.hip behind include/pixelsynth_lmconv_bwd.h): grad_weight and grad_bias are one GEMM over the
B*L locations on the same MFMA, and grad_input is the forward kernel itself on the adjoint mask and the flipped,
transposed weight.  No CPU fallback, no atomics: a backward pass gives the same bits every time.
"""
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable
from torch.nn.parameter import Parameter

from .. import _lib

_WS = _lib.Workspace()     # lmconv's own: the forward's and the backward's scratch, whichever is larger


def compact_mask(mask, B, C_in):
    """The reference hands the mask repeated C_in times, (B*C_in, 9, L), identical across channels
    (models/z_buffermodel.py:697-699).  Returns one copy per image (B|1, 9, L), contiguous f32."""
    if mask.dim() != 3:
        raise ValueError("mask must be (B*C_in, k1*k2, L), (B, k1*k2, L) or (1, k1*k2, L)")
    if mask.size(0) == B * C_in and C_in > 1:
        mask = mask.view(B, C_in, mask.size(1), mask.size(2))[:, 0]
    elif mask.size(0) not in (1, B):
        raise ValueError(f"mask batch {mask.size(0)} matches neither B={B} nor B*C_in={B * C_in}")
    return mask.float().contiguous()


def lmconv_forward(x, mask, weight, bias=None, dilation=1):
    """y[b,o,l] = bias[o] + sum_{c,t} W[o,c,t] * mask[b,t,l] * xpad[b,c,l+dil*off(t)]  (reference :25-49)."""
    if x.dim() != 4:
        raise AssertionError("lmconv expects a 4D (B, C, H, W) input")
    out_channels, in_channels, k1, k2 = weight.shape
    if x.size(1) != in_channels or mask.size(1) != k1 * k2:
        raise AssertionError(f"lmconv: input has {x.size(1)} channels / mask {mask.size(1)} taps, "
                             f"weight wants {in_channels} / {k1 * k2}")
    if (k1, k2) != (3, 3):
        raise NotImplementedError("the HIP lmconv kernel implements the 3x3 kernels PixelSynth uses")
    B, _, H, W = x.shape
    m = compact_mask(mask, B, in_channels)
    stride = 0 if m.size(0) == 1 and B > 1 else 9 * H * W
    xc = x.float().contiguous()
    wc = weight.float().contiguous()
    bc = None if bias is None else bias.float().contiguous()
    y = torch.empty(B, out_channels, H, W, dtype=torch.float32, device=x.device)
    ws = _WS.get(x.device, _lib.call("ps_lmconv_workspace_bytes", B, in_channels, out_channels, H, W))
    _lib.call("ps_lmconv_forward_f32", xc, m, stride, wc, bc, B, in_channels, out_channels, H, W, int(dilation), y, ws, ws.numel())
    return y


def adjoint_mask(m, H, W, dilation=1):
    """m (B|1,9,L) contiguous f32 on the device -> m'[b,t,p] = m[b,8-t,p+off(t)] inside the grid, 0 outside: the mask with which
    grad_x = lmconv_forward(grad_y, m', weight.flip(2, 3).transpose(0, 1))."""
    out = torch.empty_like(m)
    _lib.call("ps_lmconv_adjoint_mask_f32", m, m.size(0), H, W, int(dilation), out)
    return out


def lmconv_backward(grad_y, x, mask, weight, dilation=1, need_x=True, need_weight=True, need_bias=False):
    """The gradients of lmconv_forward for grad_y (B,Co,H,W): -> (grad_x (B,Ci,H,W), grad_weight (Co,Ci,3,3) summed over the batch,
    grad_bias (Co)), None for what is not asked for.  mask in any form compact_mask accepts."""
    _lib.require_cuda(grad_y, x, mask, weight)
    B, Ci, H, W = x.shape
    Co = weight.size(0)
    if tuple(weight.shape[1:]) != (Ci, 3, 3) or tuple(grad_y.shape) != (B, Co, H, W):
        raise AssertionError(f"lmconv backward: grad_output {tuple(grad_y.shape)} / weight {tuple(weight.shape)} for an input {tuple(x.shape)}")
    m = compact_mask(mask, B, Ci)
    g = grad_y.float().contiguous()            # (y.sum().backward() hands over a stride-0 expansion)
    gx = gw = gb = None
    with torch.cuda.device(x.device):
        if need_x:
            gx = lmconv_forward(g, adjoint_mask(m, H, W, dilation), weight.detach().flip(2, 3).transpose(0, 1), None, dilation)
        if need_weight or need_bias:
            stride = 0 if m.size(0) == 1 and B > 1 else 9 * H * W
            gw = torch.empty(Co, Ci, 3, 3, dtype=torch.float32, device=x.device) if need_weight else None
            gb = torch.empty(Co, dtype=torch.float32, device=x.device) if need_bias else None
            ws = _WS.get(x.device, _lib.call("ps_lmconv_bwd_workspace_bytes", B, Ci, Co, H, W)) if need_weight else None
            _lib.call("ps_lmconv_grad_weight_f32", x.detach().float().contiguous() if need_weight else None, g, m if need_weight else None,
                      stride, B, Ci, Co, H, W, int(dilation), gw, gb, ws, ws.numel() if need_weight else 0)
    return gx, gw, gb


class _locally_masked_conv2d(torch.autograd.Function):
    """Same call surface as the reference autograd.Function; forward is lmconv_forward, backward lmconv_backward."""

    @staticmethod
    def forward(ctx, x, mask, weight, mask_weight=None, bias=None, dilation=1, padding=1):
        if mask_weight is not None:
            raise NotImplementedError("conv_mask_weight=True is not used by PixelSynth (z_buffermodel.py:71)")
        if ctx.needs_input_grad[1]:
            raise AssertionError("lmconv: the mask takes no gradient (the reference's backward asserts it, :91)")
        ctx.save_for_backward(x, mask, weight)
        ctx.dilation, ctx.has_bias = dilation, bias is not None
        return lmconv_forward(x, mask, weight, bias, dilation)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, mask, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gw, gb = lmconv_backward(grad_output, x, mask, weight, ctx.dilation, need[0], need[2], ctx.has_bias and need[4])
        cast = lambda g, like: g if g is None or g.dtype == like.dtype else g.to(like.dtype)
        return cast(gx, x), None, cast(gw, weight), None, gb, None, None


class locally_masked_conv2d(nn.Module):
    """Module form: parameters `weight (Co,Ci,k,k)`, optional `mask_weight (Co,k,k)` and `bias (Co)` under the
    reference's names, default-initialised like a torch conv (uniform with bound 1/sqrt(fan_in))."""

    def __init__(self, in_channels, out_channels, kernel_size=(3, 3), dilation=1, bias=True, mask_weight=False):
        super(locally_masked_conv2d, self).__init__()
        kh, kw = kernel_size
        self.in_channels, self.out_channels, self.dilation = in_channels, out_channels, dilation
        self.padding = tuple(dilation * (k - 1) // 2 for k in (kh, kw))
        self.weight = Parameter(torch.empty(out_channels, in_channels, kh, kw))
        self.mask_weight = Parameter(torch.empty(out_channels, kh, kw)) if mask_weight else None
        self.bias = Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels * self.weight.shape[2] * self.weight.shape[3])
        with torch.no_grad():
            for p_ in (self.weight, self.mask_weight):
                if p_ is not None:
                    nn.init.kaiming_uniform_(p_, a=math.sqrt(5))      # = U(-1/sqrt(fan_in), +1/sqrt(fan_in))
            if self.bias is not None:
                self.bias.uniform_(-bound, bound)

    def forward(self, x, mask=None):
        return _locally_masked_conv2d.apply(x, mask, self.weight, self.mask_weight, self.bias, self.dilation,
                                            self.padding)
