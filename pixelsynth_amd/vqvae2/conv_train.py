"""The VQ-VAE's convolutions in training (vqvae2/vqvae.py under vqvae_train("hip")): torch.autograd.Functions, once differentiable, whose
forward passes are bit for bit what _FastPath computes with the same weights -- a model trains on the arithmetic it runs at inference --
and whose backward passes run on the matrix products that exist already (csrc/conv_f16x3.hip, csrc/conv_bwd.hip, csrc/conv1x1.hip,
csrc/block_train.hip) with the passes of csrc/vq_conv_train.hip (libpixelsynth_vq_conv_train.so) around them.

conv3x3_relu_train(x, w, b, relu_in)          Conv2d(Ci, Co, 3, 1, 1) on relu(x) or x
conv4x4s2_train(x, w, b, relu_in, x_is_s2d)   Conv2d(Ci, Co, 4, 2, 1): a 3 x 3 convolution over the 2 x 2 blocks of its input (s2d_weight);
                                              its input gradient is the transposed convolution of the same tensor, run towards the four
                                              output parities (convt_weight); its weight gradient the 3 x 3 GEMM on the blocked relu(x),
                                              folded.  x_is_s2d: x is given in blocks already (the stem's output) and its gradient leaves so
convt4x4s2_train(x, w, b, relu_in)            ConvTranspose2d(Ci, Co, 4, 2, 1): the converse of each of those
res_block_train(x, w3, b3, w1, b1)            ResBlock: conv1x1(relu(conv3x3(relu(x)))) + relu(x); the skip's gradient joins in the gate
conv1x1_relu_train(x, w, b)                   Conv2d(Ci, Co, 1) on relu(x)
stem_train(img, w, b), head_train(h, wt, b)   the two 3-channel ends (csrc/vq_ends.hip) with the backward kernels of vq_conv_train.hip

Every Function saves its raw input and its weights; relu(x), the blocked copy and the packed weights are rebuilt in the backward pass.
The gradient of a layer's output is scaled by a power of two on the device (f16x3.bwd_prepare) and nothing is read back.  Two runs give
the same bits; a frame's result and input gradient do not depend on the batch it is in.  What a function does not take -- the CPU, fp64,
other shapes, a weight fp16 cannot hold (check=True synchronises to find out; the route below has looked at all weights at once and
passes check=False with the scale below) -- raises ValueError and the caller goes through torch.  An activation beyond fp16's range raises f16x3.flag(device)
as in the no-grad route: check_f16x3_overflow() is the caller's (vqvae2/train.py calls it before the optimiser steps).

The weights of this network are small (0.03 and less), and below 2^-3 the low half of conv_f16x3.hip's operand split is a subnormal fp16:
a weight is then held to 2^-25 absolute, about 1e-6 of itself, the same error at every pixel, which adds up along a backward pass of
fourteen layers.  The forward pass keeps that arithmetic -- it is the fast path's --, but the grad-input pass packs its flipped weight
multiplied by a power of two (weight_scale: the largest magnitude into [2^14, 2^15), as bwd_prepare does for the gradient) and the gate
multiplies by its inverse, both exact.

forward_train(m, input) is VQVAETop.forward on these, takes(m, input) what it asks of the module and the call.
"""
import math

import torch
from torch.nn import functional as F

from .. import _lib
from ..networks import block_train
from ..networks.block_train import conv1x1_train
from ..networks.f16x3 import bwd_prepare, conv3x3, flag, forced_mode, grad_flag, grad_input, pack3x3, plain_relu, train_takes
from ..networks.routing import empty_nhwc, gpu_f32, grad_nhwc
from . import vqvae as V

_WS = _lib.Workspace()        # the grad-weight GEMM of a transposed layer (its sizes are not bwd_prepare's)
_WS1 = _lib.Workspace()       # the 1 x 1 grad-weight GEMMs
_WSE = _lib.Workspace()       # the ends


# ---- the passes of csrc/vq_conv_train.hip ------------------------------------------------------------------------------------------------
def relu_pack(x, relu, s2d):
    """relu(x) or x of x (B, C, H, W) channels_last, as it lies or as its 2 x 2 blocks (B, 4 C, H / 2, W / 2) in _s2d's channel order"""
    B, C, H, W = x.shape
    out = empty_nhwc(B, 4 * C, H // 2, W // 2, x) if s2d else empty_nhwc(B, C, H, W, x)
    _lib.call("ps_vq_relu_pack_f32", x, B, H, W, C, int(relu), int(s2d), out)
    return out


def gate(gx, x=None, skip=None, scale2=None):
    """In place: gx = (x > 0) ? (gx * scale2[1] + skip) : 0, each of the three absent where its operand is None -> gx"""
    _lib.call("ps_vq_gate_f32", gx, x, skip, scale2, gx.numel())
    return gx


def fold(g, Co, Ci, transposed):
    """(Co, 3, 3, 4 Ci) -> (Co, Ci, 4, 4), or transposed (4 Co, 3, 3, Ci) -> (Ci, Co, 4, 4): the live taps of s2d_weight / convt_weight"""
    out = torch.empty((Ci, Co, 4, 4) if transposed else (Co, Ci, 4, 4), dtype=torch.float32, device=g.device)
    _lib.call("ps_vq_fold_f32", g, Co, Ci, int(transposed), out)
    return out


def _grad_weight(x, gs, scale2, ws):
    """ps_conv3x3_grad_weight_f16x3 of x (B, Ci, H, W) and the scaled gradient gs (B, Co, H, W) -> (Co, 3, 3, Ci)"""
    B, Ci, H, W = x.shape
    Co = gs.size(1)
    gw = torch.empty((Co, 3, 3, Ci), dtype=torch.float32, device=x.device)
    _lib.call("ps_conv3x3_grad_weight_f16x3", x, gs, scale2, B, H, W, Ci, Co, gw, flag(x.device), ws, ws.numel())
    return gw


def weight_scale(top):
    """The power of two that brings a largest magnitude `top` into [2^14, 2^15), its exponent held in [-16, 40]; 1 for 0.  ValueError for
    what fp16 cannot hold (6e4 or more, or not a number), as f16x3.check_weight"""
    if not (top == top and top < 6.0e4):
        raise ValueError("split-fp16 convolution: a weight fp16 cannot hold")
    return 2.0 ** max(-16, min(40, 15 - math.frexp(top)[1])) if top > 0 else 1.0


_wmul = {}      # (device, scale) -> (1, 1 / scale) on the device


def _unscale(scale2, wscale):
    """bwd_prepare's (s, 1 / s) with the inverse of the weight's scale folded into the second"""
    if wscale == 1.0:
        return scale2
    key = (str(scale2.device), wscale)
    if key not in _wmul:
        _wmul[key] = torch.tensor([1.0, 1.0 / wscale], dtype=torch.float32, device=scale2.device)
    return scale2 * _wmul[key]


def _weight_ok(x, w, shape, what):
    if not (w.dim() == len(shape) and tuple(w.shape) == tuple(shape) and w.dtype == torch.float32 and w.device == x.device):
        raise ValueError(f"{what}: weight {tuple(w.shape)}, {tuple(shape)} fp32 on x's device required")


def _bias_ok(x, b, n, what):
    if b is not None and not (tuple(b.shape) == (n,) and b.dtype == torch.float32 and b.device == x.device):
        raise ValueError(f"{what}: bias must be ({n}) fp32 on x's device")


def _x_ok(x, what):
    if not (gpu_f32(x, aligned=True) and x.numel() > 0):
        raise ValueError(f"{what}: x must be a channels_last fp32 tensor (B, C, H, W) on the device")


def _bias(b):
    return None if b is None else b.detach().contiguous()


# ---- the 3 x 3 forms ---------------------------------------------------------------------------------------------------------------------
PLAIN, S2D, BLOCKED, D2S = "plain", "s2d", "blocked", "d2s"


class _ConvForm(torch.autograd.Function):
    """One layer of conv_f16x3.hip in one of its four forms.  PLAIN: w (Co, Ci, 3, 3).  S2D: w (Co, Ci, 4, 4) of a stride-2 convolution on
    x (B, Ci, H, W), read in blocks by the kernel.  BLOCKED: the same on x given in blocks (B, 4 Ci, H / 2, W / 2).  D2S: w (Ci, Co, 4, 4) of a
    transposed convolution, the four output parities stored where they belong."""

    @staticmethod
    def forward(ctx, x, w, b, relu_in, form, wscale):
        wd = w.detach()
        if form == D2S:
            p = pack3x3(V.convt_weight(wd), None if b is None else b.detach().repeat(4), d2s=True, check=False)
        elif form == PLAIN:
            p = pack3x3(wd, _bias(b), check=False)
        else:
            p = pack3x3(V.s2d_weight(wd), _bias(b), s2d=form == S2D, check=False)
        y = conv3x3(x, p, *(plain_relu(x.size(0), p["Ci"], x.device) if relu_in else ()))
        ctx.save_for_backward(x, w)
        ctx.relu_in, ctx.form, ctx.has_bias, ctx.wscale = relu_in, form, b is not None, wscale
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        relu_in, form = ctx.relu_in, ctx.form
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        wd, dev = w.detach(), x.device
        wb = wd * ctx.wscale if need_x and ctx.wscale != 1.0 else wd          # the weight of the grad-input pass (module docstring)
        g = grad_nhwc(grad_y)
        B = x.size(0)
        gx = gw = None
        if form in (PLAIN, BLOCKED):
            gs, scale2, gb, ws = bwd_prepare(g, x.size(1), need_b)
            if need_w:
                gw = _grad_weight(relu_pack(x, True, False) if relu_in else x, gs, scale2, ws)
                gw = gw.permute(0, 3, 1, 2) if form == PLAIN else fold(gw, w.size(0), w.size(1), False)
            if need_x:
                w3 = wb if form == PLAIN else V.s2d_weight(wb)
                gx = grad_input(gs, pack3x3(w3.flip(2, 3).transpose(0, 1), check=False))
        elif form == S2D:
            Co, Ci = w.shape[:2]
            gs, scale2, gb, ws = bwd_prepare(g, 4 * Ci, need_b)
            if need_w:
                gw = fold(_grad_weight(relu_pack(x, relu_in, True), gs, scale2, ws), Co, Ci, False)
            if need_x:      # the adjoint: the transposed convolution of the same tensor, towards the four parities of x's pixels
                gx = conv3x3(gs, pack3x3(V.convt_weight(wb), d2s=True, check=False), overflow=grad_flag(dev))
        else:
            Ci, Co = w.shape[:2]
            gs, scale2, gb, _ = bwd_prepare(g, Ci, need_b)
            if need_w:
                ws = _WS.query(dev, "ps_conv3x3_bwd_workspace_bytes", B, x.size(2), x.size(3), Ci, 4 * Co)
                gw = fold(_grad_weight(relu_pack(x, True, False) if relu_in else x, relu_pack(gs, False, True), scale2, ws), Co, Ci, True)
            if need_x:      # the adjoint: the stride-2 convolution of the same tensor, over the 2 x 2 blocks of the gradient
                gx = conv3x3(gs, pack3x3(V.s2d_weight(wb), s2d=True, check=False), overflow=grad_flag(dev))
        if need_x:
            gate(gx, x if relu_in else None, None, _unscale(scale2, ctx.wscale))
        return gx, gw, gb, None, None, None


def _conv_form(what, x, w, b, relu_in, form, check, wscale):
    _x_ok(x, what)
    B, C, H, W = x.shape
    if form == PLAIN:
        Ci, Co, shape, ok = C, w.size(0), (w.size(0), C, 3, 3), train_takes(C, w.size(0), H, W)
    elif form == BLOCKED:
        Ci, Co, shape = C // 4, w.size(0), (w.size(0), C // 4, 4, 4)
        ok = C % 256 == 0 and train_takes(C, Co, H, W)
    elif form == S2D:
        Ci, Co, shape = C, w.size(0), (w.size(0), C, 4, 4)
        ok = H % 2 == 0 and W % 2 == 0 and train_takes(4 * C, Co, H // 2, W // 2) and C % 64 == 0
    else:
        Ci, Co, shape = C, w.size(1) if w.dim() == 4 else 0, (C, w.size(1) if w.dim() == 4 else 0, 4, 4)
        ok = train_takes(C, 4 * Co, H, W) and Co % 64 == 0
    if w.dim() != 4 or not ok:
        raise ValueError(f"{what}: weight {tuple(w.shape)} on x {tuple(x.shape)}: channel counts multiples of 64 and output sides "
                         "multiples of 16 required")
    _weight_ok(x, w, shape, what)
    _bias_ok(x, b, Co, what)
    if check:
        wscale = weight_scale(float(w.detach().abs().max()))
    return _ConvForm.apply(x, w, b, bool(relu_in), form, float(wscale))


def conv3x3_relu_train(x, w, b, relu_in, check=True, wscale=1.0):
    """conv2d(relu(x) or x, w, b, stride 1, padding 1): x (B, Ci, H, W) channels_last fp32 on the device, w (Co, Ci, 3, 3), Ci and Co
    multiples of 64, H and W multiples of 16.  check=True (here and below): the weight's range is read back (one synchronisation) and
    its scale for the grad-input pass taken from it; check=False: the caller has looked and gives `wscale`, a power of two"""
    return _conv_form("conv3x3_relu_train", x, w, b, relu_in, PLAIN, check, wscale)


def conv4x4s2_train(x, w, b, relu_in, x_is_s2d=False, check=True, wscale=1.0):
    """conv2d(relu(x) or x, w, b, stride 2, padding 1), w (Co, Ci, 4, 4), Ci and Co multiples of 64, output sides multiples of 16:
    x (B, Ci, H, W) channels_last, or with x_is_s2d its 2 x 2 blocks (B, 4 Ci, H / 2, W / 2) -> (B, Co, H / 2, W / 2)"""
    return _conv_form("conv4x4s2_train", x, w, b, relu_in, BLOCKED if x_is_s2d else S2D, check, wscale)


def convt4x4s2_train(x, w, b, relu_in, check=True, wscale=1.0):
    """conv_transpose2d(relu(x) or x, w, b, stride 2, padding 1), w (Ci, Co, 4, 4), Ci and Co multiples of 64, x's sides multiples of
    16 -> (B, Co, 2 H, 2 W)"""
    return _conv_form("convt4x4s2_train", x, w, b, relu_in, D2S, check, wscale)


# ---- the 1 x 1 convolution behind a ReLU -----------------------------------------------------------------------------------------------------
def _conv1x1_grad_weight(x, g, Ci, Co, bias):
    """block_train's GEMM over the pixels of x (npix, Ci) and g (npix, Co) -> ((Co, Ci), (Co) or None)"""
    npix = x.numel() // Ci
    ws = _WS1.query(x.device, "ps_conv1x1_grad_weight_workspace_bytes", npix, Ci, Co)
    gw = torch.empty((Co, Ci), dtype=torch.float32, device=x.device)
    gb = torch.empty(Co, dtype=torch.float32, device=x.device) if bias else None
    _lib.call("ps_conv1x1_grad_weight_f32", x, g, npix, Ci, Co, gw, gb, ws, ws.numel())
    return gw, gb


class _Conv1x1Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        B, Ci, H, W = x.shape
        Co = w.size(0)
        y = empty_nhwc(B, Co, H, W, x)
        _lib.call("ps_conv1x1_ex_nhwc_f32", x, Ci, w.detach().reshape(Co, Ci).contiguous(), _bias(b), None, 1, B * H * W, Ci, Co, y)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co, npix = w.size(0), B * H * W
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g = grad_nhwc(grad_y)
        gx = gw = gb = None
        if need_x:
            gx = torch.empty_like(x)
            _lib.call("ps_conv1x1_nhwc_f32", g, w.detach().reshape(Co, Ci).t().contiguous(), npix, Co, Ci, gx)
            gate(gx, x)
        if need_w or need_b:
            gw, gb = _conv1x1_grad_weight(relu_pack(x, True, False), g, Ci, Co, need_b)
            gw = gw.view(w.shape) if need_w else None
        return gx, gw, gb


def conv1x1_relu_train(x, w, b=None):
    """conv2d(relu(x), w, b) for a 1 x 1 weight (Co, Ci, 1, 1) or (Co, Ci) (any strides): the sizes block_train.conv1x1_takes takes both ways"""
    what = "conv1x1_relu_train"
    _x_ok(x, what)
    Ci = x.size(1)
    if not (w.dim() in (2, 4) and w.shape[:2] == (w.size(0), Ci) and w.numel() == w.size(0) * Ci and w.dtype == torch.float32
            and w.device == x.device and block_train.conv1x1_takes(Ci, w.size(0), x.numel() // Ci)
            and _lib.call("ps_conv1x1_takes", w.size(0), Ci)):
        raise ValueError(f"{what}: weight {tuple(w.shape)} on x {tuple(x.shape)}: sizes csrc/conv1x1.hip takes both ways required")
    _bias_ok(x, b, w.size(0), what)
    return _Conv1x1Relu.apply(x, w, b)


# ---- the ResBlock ------------------------------------------------------------------------------------------------------------------------
PAD = 64      # the middle channels as conv_f16x3.hip packs them


class _ResBlock(torch.autograd.Function):
    """_FastPath.res's two launches.  Saved: x, the weights and h, the raw input of the inner 1 x 1 layer (PAD channels, the first `mid`
    live, the others zero)."""

    @staticmethod
    def forward(ctx, x, w3, b3, w1, b1, wscale):
        B, C, H, W = x.shape
        mid = w3.size(0)
        ctx.wscale = wscale
        h = conv3x3(x, pack3x3(w3.detach(), _bias(b3), check=False), *plain_relu(B, C, x.device))
        y = empty_nhwc(B, C, H, W, x)
        _lib.call("ps_conv1x1_ex_nhwc_f32", h, h.size(1), w1.detach().reshape(C, mid).contiguous(), _bias(b1), x, 3, B * H * W, mid, C, y)
        ctx.save_for_backward(x, w3, w1, h)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, w3, w1, h = ctx.saved_tensors
        B, C, H, W = x.shape
        mid, npix, dev = w3.size(0), B * H * W, x.device
        need_x, need_w3, need_b3, need_w1, need_b1 = ctx.needs_input_grad[:5]
        g = grad_nhwc(grad_y)
        gx = gw3 = gb3 = gw1 = gb1 = None
        # the 1 x 1 layer on relu(h): the pad rows of its weight are zeros, their gradients are dropped
        if need_w1 or need_b1:
            gw1, gb1 = _conv1x1_grad_weight(relu_pack(h, True, False), g, PAD, C, need_b1)
            gw1 = gw1[:, :mid].reshape(w1.shape) if need_w1 else None
        if not (need_x or need_w3 or need_b3):
            return None, None, None, gw1, gb1, None
        w1t = torch.zeros((PAD, C), dtype=torch.float32, device=dev)
        w1t[:mid] = w1.detach().reshape(C, mid).t()
        gh = torch.empty_like(h)
        _lib.call("ps_conv1x1_nhwc_f32", g, w1t, npix, C, PAD, gh)
        gate(gh, h)
        # the 3 x 3 layer on relu(x), PAD output channels
        gs, scale2, gb3, ws = bwd_prepare(gh, C, need_b3)
        if need_b3:
            gb3 = gb3[:mid]
        if need_w3:
            gw3 = _grad_weight(relu_pack(x, True, False), gs, scale2, ws)[:mid].permute(0, 3, 1, 2)
        if need_x:
            w3p = torch.cat([w3.detach() * ctx.wscale, w3.new_zeros(PAD - mid, C, 3, 3)])
            gx = grad_input(gs, pack3x3(w3p.flip(2, 3).transpose(0, 1), check=False))
            gate(gx, x, g, _unscale(scale2, ctx.wscale))          # + the skip's gradient, then relu(x)'s mask on both
        return gx, gw3, gb3, gw1, gb1, None


def res_block_train(x, w3, b3, w1, b1, check=True, wscale=1.0):
    """ResBlock: conv2d(relu(conv2d(relu(x), w3, b3, 1, 1)), w1, b1) + relu(x); x (B, C, H, W) channels_last fp32 on the device, C a
    multiple of 64, H and W multiples of 16, w3 (mid, C, 3, 3) with mid a multiple of 16 up to 64, w1 (C, mid, 1, 1), both biases given"""
    what = "res_block_train"
    _x_ok(x, what)
    B, C, H, W = x.shape
    mid = w3.size(0) if w3.dim() == 4 else 0
    if not (0 < mid <= PAD and mid % 16 == 0 and train_takes(C, PAD, H, W) and _lib.call("ps_conv1x1_takes", mid, C)
            and _lib.call("ps_conv1x1_takes", C, PAD) and block_train.conv1x1_takes(PAD, C, B * H * W)):
        raise ValueError(f"{what}: {C} channels with {mid} in the middle on {H} x {W}: sizes the kernels do not take")
    _weight_ok(x, w3, (mid, C, 3, 3), what)
    _weight_ok(x, w1, (C, mid, 1, 1), what)
    if b3 is None or b1 is None:
        raise ValueError(f"{what}: both biases required")
    _bias_ok(x, b3, mid, what)
    _bias_ok(x, b1, C, what)
    if check:
        wscale = weight_scale(float(w3.detach().abs().max()))
    return _ResBlock.apply(x, w3, b3, w1, b1, float(wscale))


# ---- the 3-channel ends ------------------------------------------------------------------------------------------------------------------
def _ends_grad_weight(img, wide, B, H, W, blocked, bias):
    ws = _WSE.query(img.device, "ps_vq_conv_train_workspace_bytes", B * (H // 2) * (W // 2))
    gw = torch.empty((64, 3, 4, 4), dtype=torch.float32, device=img.device)
    gb = torch.empty(64 if blocked else 3, dtype=torch.float32, device=img.device) if bias else None
    _lib.call("ps_vq_ends_grad_weight_f32", img, wide, B, H, W, int(blocked), gw, gb, ws, ws.numel())
    return gw, gb


class _Stem(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, w, b):
        B, _, H, W = img.shape
        s = torch.empty((B, H // 4, W // 4, 256), dtype=torch.float32, device=img.device)
        _lib.call("ps_vq_stem_s2d_f32", img, w.detach().contiguous(), b.detach().contiguous(), B, H, W, s)
        ctx.save_for_backward(img)
        return s.permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_s):
        img, = ctx.saved_tensors
        B, _, H, W = img.shape
        if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None
        gw, gb = _ends_grad_weight(img, grad_nhwc(grad_s), B, H, W, True, ctx.needs_input_grad[2])
        return None, gw if ctx.needs_input_grad[1] else None, gb


def stem_train(img, w, b):
    """Conv2d(3, 64, 4, 2, 1) of img (B, 3, H, W) NCHW fp32 on the device, H a multiple of 4 and W of 16, WITH its bias -> the 2 x 2
    blocks of its output (B, 256, H / 4, W / 4) channels_last, as conv4x4s2_train(x_is_s2d=True) reads them.  The image gets no gradient."""
    what = "stem_train"
    if not (gpu_f32(img, layout=torch.contiguous_format, aligned=True) and img.numel() > 0 and img.size(1) == 3 and img.size(2) % 4 == 0
            and img.size(3) % 16 == 0 and img.numel() // 12 < 2 ** 31):
        raise ValueError(f"{what}: img must be a contiguous fp32 (B, 3, H, W) on the device, H a multiple of 4 and W of 16")
    if img.requires_grad:
        raise ValueError(f"{what}: the image takes no gradient")
    _weight_ok(img, w, (64, 3, 4, 4), what)
    if b is None:
        raise ValueError(f"{what}: a bias is required")
    _bias_ok(img, b, 64, what)
    return _Stem.apply(img, w, b)


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, wt, b):
        B, _, Hh, Wh = h.shape
        img = torch.empty((B, 3, 2 * Hh, 2 * Wh), dtype=torch.float32, device=h.device)
        _lib.call("ps_vq_head_f32", h, wt.detach().contiguous(), b.detach().contiguous(), B, Hh, Wh, img)
        ctx.save_for_backward(h, wt)
        return img

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_img):
        h, wt = ctx.saved_tensors
        B, _, Hh, Wh = h.shape
        g = grad_img.to(torch.float32).contiguous()
        gh = gw = gb = None
        if ctx.needs_input_grad[0]:
            gh = torch.empty_like(h)
            _lib.call("ps_vq_head_grad_input_f32", g, wt.detach().contiguous(), h, B, Hh, Wh, gh)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = _ends_grad_weight(g, h, B, 2 * Hh, 2 * Wh, False, ctx.needs_input_grad[2])
            gw = gw if ctx.needs_input_grad[1] else None
        return gh, gw, gb


def head_train(h, wt, b):
    """ConvTranspose2d(64, 3, 4, 2, 1) of relu(h), h (B, 64, Hh, Wh) channels_last fp32 on the device, Wh a multiple of 16, wt (64, 3, 4, 4)
    -> the image (B, 3, 2 Hh, 2 Wh) NCHW"""
    what = "head_train"
    _x_ok(h, what)
    if not (h.size(1) == 64 and h.size(3) % 16 == 0 and h.numel() // 64 < 2 ** 31):
        raise ValueError(f"{what}: h {tuple(h.shape)}: 64 channels and a width that is a multiple of 16 required")
    _weight_ok(h, wt, (64, 3, 4, 4), what)
    if b is None:
        raise ValueError(f"{what}: a bias is required")
    _bias_ok(h, b, 3, what)
    return _Head.apply(h, wt, b)


# ---- the route: VQVAETop.forward on the Functions above ----------------------------------------------------------------------------------
def scale_for(m, input):
    """The weight scale of the call (weight_scale of the largest parameter) if forward_train takes it, else None: grad mode, the split-fp16 route in effect, a float32 CUDA image the fast path takes, fp32
    parameters on its device, the module as VQVAETop builds it (dec_t included) with the ends of csrc/vq_ends.hip, and -- one batched
    reduction and ONE read-back -- no parameter that fp16 cannot hold"""
    if not (torch.is_grad_enabled() and (forced_mode() or V.VQVAE_CONV) == "f16x3" and torch.is_tensor(input) and input.is_cuda
            and input.dtype == torch.float32 and input.dim() == 4 and input.size(1) == 3 and not input.requires_grad
            and V._FastPath.takes(m, input.size(2), input.size(3))):
        return None
    params = list(m.parameters())
    if any(p.dtype != torch.float32 or p.device != input.device for p in params):
        return None
    try:
        eb, dt, dc = m.enc_b.blocks, m.dec_t.blocks, m.dec.blocks
        ok = (len(dt) == 5 and isinstance(dt[0], torch.nn.Conv2d) and isinstance(dt[4], torch.nn.ConvTranspose2d)
              and tuple(eb[0].weight.shape) == (64, 3, 4, 4) and tuple(dc[6].weight.shape) == (64, 3, 4, 4)
              and all(c.bias is not None for c in (eb[0], dc[6])))
    except (AttributeError, IndexError, TypeError):
        return None
    if not ok:
        return None
    try:
        return weight_scale(float(torch.cat([p.detach().reshape(-1) for p in params]).abs().max()))
    except ValueError:
        return None


def takes(m, input):
    return scale_for(m, input) is not None


def _conv(c):
    return c.weight, c.bias


def _res(h, block, ws):
    return res_block_train(h, *_conv(block.conv[1]), *_conv(block.conv[3]), check=False, wscale=ws)


def enc_b_train(m, input, ws=1.0):
    """enc_b(input) BEFORE its trailing ReLU (the layers that follow apply it on the way in)"""
    eb = m.enc_b.blocks
    h = stem_train(input.contiguous(), *_conv(eb[0]))
    h = conv4x4s2_train(h, *_conv(eb[2]), True, x_is_s2d=True, check=False, wscale=ws)
    h = conv3x3_relu_train(h, *_conv(eb[4]), True, check=False, wscale=ws)
    return _res(_res(h, eb[5], ws), eb[6], ws)


def enc_t_train(m, bottom, ws=1.0):
    """quantize_conv_t(enc_t(relu(bottom))) -> (B, embed_dim, H / 8, W / 8) channels_last"""
    et = m.enc_t.blocks
    h = conv4x4s2_train(bottom, *_conv(et[0]), True, check=False, wscale=ws)
    h = conv3x3_relu_train(h, *_conv(et[2]), True, check=False, wscale=ws)
    h = _res(_res(h, et[3], ws), et[4], ws)
    return conv1x1_relu_train(h, *_conv(m.quantize_conv_t))


def encode_latent_train(m, input, ws=1.0):
    return enc_t_train(m, enc_b_train(m, input, ws), ws)


def dec_t_train(m, quant_t, ws=1.0):
    dt = m.dec_t.blocks
    h = conv3x3_relu_train(quant_t, *_conv(dt[0]), False, check=False, wscale=ws)
    h = _res(_res(h, dt[1], ws), dt[2], ws)
    return convt4x4s2_train(h, *_conv(dt[4]), True, check=False, wscale=ws)


def decode_train(m, quant_t, ws=1.0):
    """dec(upsample_t(quant_t)), quant_t (B, embed_dim, H, W) channels_last -> the image (B, 3, 8 H, 8 W)"""
    dc = m.dec.blocks
    h = convt4x4s2_train(quant_t, *_conv(m.upsample_t), False, check=False, wscale=ws)
    h = conv3x3_relu_train(h, *_conv(dc[0]), False, check=False, wscale=ws)
    h = _res(_res(h, dc[1], ws), dc[2], ws)
    h = convt4x4s2_train(h, *_conv(dc[4]), True, check=False, wscale=ws)
    return head_train(h, *_conv(dc[6]))


def quantize_conv_b_train(m, dec_t_out, bottom):
    """quantize_conv_b(cat(dec_t_out, relu(bottom))) as two 1 x 1 convolutions on the weight's column blocks and an add: the
    concatenation is never built.  Through torch where csrc/conv1x1.hip refuses a block."""
    c = m.quantize_conv_b
    D = dec_t_out.size(1)
    try:
        return conv1x1_train(dec_t_out, c.weight[:, :D], c.bias) + conv1x1_relu_train(bottom, c.weight[:, D:], None)
    except ValueError:
        return c(torch.cat([dec_t_out, F.relu(bottom)], dim=1))


def forward_train(m, input, ws=1.0):
    """VQVAETop.forward(input) -> (image, diff) for a call whose scale_for(m, input) is ws; the quantisers are the module's own"""
    bottom = enc_b_train(m, input, ws)
    quant_t, diff_t, _ = m._quantise(m.quantize_t, enc_t_train(m, bottom, ws))
    _, diff_b, _ = m._quantise(m.quantize_b, quantize_conv_b_train(m, dec_t_train(m, quant_t, ws), bottom))
    return decode_train(m, quant_t, ws), diff_t + diff_b
