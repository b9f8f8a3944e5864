"""The split-fp16 3 x 3 convolution (csrc/conv_f16x3.hip) of the refinement decoder and the VQ-VAE: weight packing, the launch and the
overflow guard.  Every product is three fp16 MFMAs on split operands, so an activation beyond fp16's range (|v| > 65000, or not a number)
gives a wrong output and sets a per-device flag (csrc/conv_thin.hip's 4 -> 64 layer likewise).  checked(device, fn) reads it: the
outermost scope clears the flag (an earlier, unchecked pass's is not this pass's), runs fn, synchronises, and if the flag is set warns and
runs fn again under decoder_conv("fp32"), every convolution through torch.  Inner scopes do nothing, so a pass made of guarded calls is
checked once.  A scope must not enclose a collective: a rerun on one rank would run it twice.

Training (csrc/conv_bwd.hip, libpixelsynth_conv_bwd.so): conv3x3_train(x, weight, bias) is the plain convolution as a
torch.autograd.Function whose backward pass runs on the same matrix pipe -- grad_y scaled by a power of two on the device, grad_weight
as a GEMM over the pixels, grad_input as the forward kernel on the flipped, transposed weight.  It is opt-in for the decoder's blocks:
decoder_conv_train("f16x3"), opt.decoder_conv_train or PS_DECODER_CONV_TRAIN; the default "fp32" leaves every call where it is.

What the runners of whole networks (perceptual.py, losses/synthesis.py) share lives here too: check_weight (what fp16 cannot hold),
plain_relu (the act tables of a plain ReLU), conv3x3_thin_in (the 4 -> 64 stem) and the gradient step grad_flag / bwd_prepare / grad_input.
"""
import warnings

import torch

from .. import _lib
from .routing import Switch, empty_nhwc, gpu_f32, grad_nhwc

_flags = {}         # str(device) -> int32 (1,) overflow flag
_open = set()       # str(device) of the guarded scopes open

# with decoder_conv("fp32"): ... -- every split-fp16 convolution inside (decoder and VQ-VAE) through torch (MIOpen fp32), whatever the
# options say: how checked() reruns a pass whose split-fp16 convolutions met an activation beyond fp16's range.  The process default is
# architectures.DECODER_CONV, which the benchmark assigns.
decoder_conv = Switch("decoder_conv", "PS_DECODER_CONV", ("f16x3", "fp32"), "f16x3", __package__ + ".architectures", "DECODER_CONV",
                      attr="decoder_conv")
forced_mode = decoder_conv.forced      # the mode of the innermost decoder_conv(...) in effect, or None

# with decoder_conv_train("f16x3"): ... -- in grad mode the decoder blocks' wide 3 x 3 convolutions (Ci and Co multiples of 64, H and W
# multiples of 16) inside go through conv3x3_train; "fp32": through torch autograd, whatever the options say.
decoder_conv_train = Switch("decoder_conv_train", "PS_DECODER_CONV_TRAIN", ("f16x3", "fp32"), "fp32", __name__, "DECODER_CONV_TRAIN",
                            attr="decoder_conv_train")
DECODER_CONV_TRAIN = decoder_conv_train.from_env()   # "fp32" (training convolutions through torch autograd) | "f16x3" (conv3x3_train)
train_mode = decoder_conv_train.resolve              # which route a decoder block's 3 x 3 convolution takes in grad mode


def flag(device):
    """The overflow flag the kernels set on `device` (int32 (1,), zero when first asked for)."""
    key = str(device)
    if key not in _flags:
        _flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _flags[key]


def check_f16x3_overflow(device):
    """Synchronises.  Raises (and clears the flag) if a split-fp16 convolution met an activation beyond fp16's range since the flag was
    last cleared: its output is then wrong."""
    f = _flags.get(str(device))
    if f is not None and int(f.item()):
        f.zero_()
        raise RuntimeError("an activation beyond fp16's range (|v| > 65000, or not a number) reached a split-fp16 convolution; "
                           "PS_DECODER_CONV=fp32 (refinement decoder) / PS_VQVAE_CONV=fp32 (VQ-VAE) run everything through torch")


def checked(device, fn, check=True):
    """fn() as a guarded scope on `device` (module docstring).  check=False: a scope that nobody inside checks -- for a caller that checks
    later, or accepts the risk."""
    key = str(device)
    if key in _open:            # the outermost scope owns the check
        return fn()
    _open.add(key)
    try:
        if not check:
            return fn()
        if key in _flags:
            _flags[key].zero_()
        out = fn()
        try:
            check_f16x3_overflow(device)
        except RuntimeError as err:
            warnings.warn(f"{err}: run again in fp32")
            with decoder_conv("fp32"):
                out = fn()
        return out
    finally:
        _open.discard(key)


def check_weight(w):
    """ValueError for a weight fp16 cannot hold: a magnitude of 6e4 or more, or not a number (synchronises to find out)"""
    top = float(w.abs().max())
    if not (top == top and top < 6.0e4):
        raise ValueError("split-fp16 convolution: a weight fp16 cannot hold")


def pack3x3(weight, bias=None, s2d=False, d2s=False, check=True):
    """A (Co, Ci, 3, 3) fp32 CUDA weight (and (Co) bias) packed for conv3x3, Co padded to a multiple of 64 (the first `live` channels are
    the layer's); s2d / d2s: for a space-to-depth input (Ci / 4 a multiple of 32) / a depth-to-space output (Co / 4 a multiple of 64).
    ValueError for a shape the kernel does not take or a weight fp16 cannot hold (synchronises to find out): the caller goes through torch.
    check=False: values that were looked at before (the backward pass packs the forward's weight flipped): nothing is read back."""
    Co, Ci = weight.shape[:2]
    if Ci % 32 or (s2d and Ci % 128) or (d2s and Co % 256):
        raise ValueError(f"split-fp16 convolution: {Co} x {Ci} channels (s2d {s2d}, d2s {d2s})")
    Cop = -(-Co // 64) * 64
    if Cop != Co:
        weight = torch.cat([weight, weight.new_zeros(Cop - Co, Ci, 3, 3)])
    wl = weight.permute(0, 2, 3, 1).contiguous()       # (Co, 3, 3, Ci): no copy for a channels_last weight
    if check:
        check_weight(wl)
    packed = torch.empty(_lib.call("ps_conv3x3_f16x3_packed_bytes", Cop, Ci), dtype=torch.uint8, device=weight.device)
    _lib.call("ps_conv3x3_f16x3_pack", wl, Cop, Ci, packed)
    if bias is not None:
        bias = torch.cat([bias, bias.new_zeros(Cop - Co)]).contiguous()
    return dict(packed=packed, Ci=Ci, Co=Cop, live=Co, bias=bias, s2d=s2d, d2s=d2s)


def conv3x3(x, p, scale=None, shift=None, bias=None, res=None, overflow=None):
    """conv3x3(act(x)) + bias + res (ps_conv3x3_f16x3_ex_nhwc) of a pack3x3 layer on x (B, Ci, H, W) channels_last fp32 -- (B, Ci / 4, 2 H,
    2 W) for s2d --, act(x) = max(x * scale - shift, 0) (scale / shift (B, Ci)) or x; bias (Co) defaults to the layer's, res is NHWC.
    -> y (B, Co, H, W) channels_last, (B, Co / 4, 2 H, 2 W) for d2s.  overflow: the int32 (1,) word the kernel raises instead of flag(x.device)."""
    B, C, H, W = x.shape
    if p["s2d"]:
        C, H, W = 4 * C, H // 2, W // 2
    assert C == p["Ci"] and x.is_contiguous(memory_format=torch.channels_last)
    shape = (B, p["Co"] // 4, 2 * H, 2 * W) if p["d2s"] else (B, p["Co"], H, W)
    y = empty_nhwc(*shape, x)
    bias = p["bias"] if bias is None else bias
    _lib.call("ps_conv3x3_f16x3_ex_nhwc", x, scale, shift, p["packed"], bias, res, B, H, W, C, p["Co"], p["live"], int(p["s2d"]),
              int(p["d2s"]), y, flag(x.device) if overflow is None else overflow)
    return y


_relu_tables = {}   # str(device) -> (ones, zeros), the largest asked for so far


def plain_relu(N, C, device):
    """-> (scale, shift), (N, C) views of ones and zeros kept per device and grown on demand: a plain ReLU as conv3x3's act,
    max(x * 1 - 0, 0)"""
    key = str(device)
    if key not in _relu_tables or _relu_tables[key][0].numel() < N * C:
        _relu_tables[key] = (torch.ones(N * C, dtype=torch.float32, device=device), torch.zeros(N * C, dtype=torch.float32, device=device))
    ones, zeros = _relu_tables[key]
    return ones[:N * C].view(N, C), zeros[:N * C].view(N, C)


def conv3x3_thin_in(x, w, scale=None, shift=None):
    """conv3x3(act(x)) WITHOUT a bias of the 4 -> 64 layer (ps_conv3x3_thin_in_f16x3_nhwc: csrc/conv_thin.hip on the fp16 matrix pipe,
    raising flag(x.device) as conv3x3 does): x (B, 4, H, W) channels_last fp32, W a multiple of 16, w [ky][kx][ci of 4][co of 64] fp32,
    act as conv3x3's -> y (B, 64, H, W) channels_last"""
    B, _, H, W = x.shape
    y = empty_nhwc(B, 64, H, W, x)
    _lib.call("ps_conv3x3_thin_in_f16x3_nhwc", x, scale, shift, w, B, H, W, 64, y, flag(x.device))
    return y


# ---- training: the plain convolution with its backward pass (csrc/conv_bwd.hip) ------------------------------------------------------------
_WS = _lib.Workspace()
_grad_flags = {}    # str(device) -> int32 (1,), see grad_flag


def grad_flag(device):
    """The word the forward kernel raises on `device` while it convolves a GRADIENT (int32 (1,)); never read: see _Conv3x3Train"""
    key = str(device)
    if key not in _grad_flags:
        _grad_flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _grad_flags[key]


def bwd_prepare(g, Ci, bias=False):
    """The first step of a convolution's backward pass (ps_conv3x3_bwd_prepare_f32) on its output's gradient g (B, Co, H, W) channels_last
    fp32, Ci the convolution's input channels -> (gs, g scaled by a power of two; scale2 (2,), the scale and its inverse on the device;
    gb (Co), the bias's gradient, or None without `bias`; ws, the workspace the grad_weight kernel goes on with)"""
    B, Co, H, W = g.shape
    ws = _WS.query(g.device, "ps_conv3x3_bwd_workspace_bytes", B, H, W, Ci, Co)
    gs = torch.empty_like(g)                                                              # (preserves channels_last)
    scale2 = torch.empty(2, dtype=torch.float32, device=g.device)
    gb = torch.empty(Co, dtype=torch.float32, device=g.device) if bias else None
    _lib.call("ps_conv3x3_bwd_prepare_f32", g, B, H, W, Co, gs, scale2, gb, ws, ws.numel())
    return gs, scale2, gb, ws


def grad_input(gs, flipped):
    """The gradient to a convolution's input, still multiplied by bwd_prepare's scale: the forward kernel on the scaled gradient gs and
    `flipped`, the pack3x3 of W'[c, t, o] = W[o, 8 - t, c]; what it raises goes to grad_flag"""
    return conv3x3(gs, flipped, overflow=grad_flag(gs.device))


def train_takes(Ci, Co, H, W):
    """The sizes conv3x3_train takes: H and W multiples of 16, Ci and Co multiples of 64, a frame within 32-bit offsets"""
    return Ci > 0 and Co > 0 and Ci % 64 == 0 and Co % 64 == 0 and H > 0 and W > 0 and H % 16 == 0 and W % 16 == 0 and H * W * max(Ci, Co) < 2 ** 31


class _Conv3x3Train(torch.autograd.Function):
    """The forward pass is pack3x3 + conv3x3: the bits of the no-grad route.  x and the weight are saved, no packed copy.  The backward
    pass reads nothing back and does not synchronise: grad_y is scaled on the device by the power of two that brings its largest
    magnitude into [2^14, 2^15) (gradients are far below the 2^-3 down to which the fp16 split keeps its 22 bits), the results are
    multiplied by its inverse.  grad_input is the forward kernel on the scaled grad_y with W'[c, t, o] = W[o, 8 - t, c]; what that kernel
    raises for a gradient that is not finite goes to a word of its own -- the outputs it reaches are not finite, which is there to see, and
    flag(device) keeps speaking of activations alone (the grad_weight kernel raises it for an x beyond fp16's range, as the forward did)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        y = conv3x3(x, pack3x3(weight.detach()), bias=None if bias is None else bias.detach().contiguous())
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co, dev = weight.size(0), x.device
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        gs, scale2, gb, ws = bwd_prepare(grad_nhwc(grad_y), Ci, need_b)
        gx = gw = None
        if need_w:
            gw = torch.empty((Co, 3, 3, Ci), dtype=torch.float32, device=dev)
            _lib.call("ps_conv3x3_grad_weight_f16x3", x, gs, scale2, B, H, W, Ci, Co, gw, flag(dev), ws, ws.numel())
            gw = gw.permute(0, 3, 1, 2)                                                   # (Co, Ci, 3, 3): a view
        if need_x:
            flipped = pack3x3(weight.detach().flip(2, 3).transpose(0, 1), check=False)    # (the forward's pack3x3 looked at these values)
            gx = grad_input(gs, flipped)
            _lib.call("ps_conv3x3_bwd_unscale_f32", gx, gx.numel(), scale2)
        return gx, gw, gb


def conv3x3_train(x, weight, bias=None):
    """conv2d(x, weight, bias, stride 1, padding 1) through the split-fp16 kernel, differentiable once in x, weight and bias.
    x (B, Ci, H, W) channels_last fp32 on the device, weight (Co, Ci, 3, 3) in any memory format, bias (Co) or None; train_takes(Ci, Co,
    H, W) sizes.  ValueError for anything else, or for a weight fp16 cannot hold (the forward's pack3x3 synchronises to find out): the
    caller goes through torch.  An activation beyond fp16's range raises flag(x.device), as in the no-grad route: checked() or
    check_f16x3_overflow() is the caller's."""
    if not gpu_f32(x):
        raise ValueError("conv3x3_train: x must be a channels_last fp32 tensor (B, Ci, H, W) on the device")
    if not (weight.dim() == 4 and tuple(weight.shape[1:]) == (x.size(1), 3, 3) and weight.dtype == torch.float32 and weight.device == x.device
            and train_takes(x.size(1), weight.size(0), x.size(2), x.size(3))):
        raise ValueError(f"conv3x3_train: weight {tuple(weight.shape)} on x {tuple(x.shape)}: (Co, Ci, 3, 3) fp32 on x's device, Ci and Co "
                         "multiples of 64, H and W multiples of 16 required")
    if bias is not None and not (bias.shape == (weight.size(0),) and bias.dtype == torch.float32 and bias.device == x.device):
        raise ValueError("conv3x3_train: bias must be (Co) fp32 on x's device")
    return _Conv3x3Train.apply(x, weight, bias)
