"""Which kernel a convolution of the refinement decoder gets (the blocks' dataflow is architectures.py's): the weight a module's forward
would use, taken apart only where that is safe (_plain_conv_weight) and cached per module (routing.cached); the batch cut of what still goes
through torch (_conv2d_batches); the no-grad routes -- conv1x1 (csrc/conv1x1.hip), _thin_conv (csrc/conv_thin.hip), _f16x3_conv
(csrc/conv_f16x3.hip through f16x3.py) --; the three training routes behind one gate (_train_route) and the depth Unet's
(_unet_train_conv); and the join of a block's branches
(_resample_sum, csrc/nets.hip).  Every route returns None for what it does not take and the caller goes on to the next; _conv_split ends
at the module's own forward."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.spectral_norm import SpectralNorm

from .. import _lib
from . import block_train, f16x3, thin_train, unet_train
from .f16x3 import flag as _overflow_flag  # noqa: F401  (architectures.py hands it on)
from .routing import cached, empty_nhwc, gpu_f32, has_pending, take_pending

_conv_mode = f16x3.decoder_conv.resolve      # which convolutions a decoder block takes: "f16x3" | "fp32" (everything through torch / MIOpen)


def plain_conv(conv, k, pad):
    """Whether `conv` is a k x k nn.Conv2d (no subclass) with stride 1, padding `pad`, no dilation and one group: what every kernel here
    computes"""
    return (type(conv) is nn.Conv2d and conv.kernel_size == (k, k) and conv.stride == (1, 1) and conv.padding == (pad, pad)
            and conv.dilation == (1, 1) and conv.groups == 1)


def _sn_hooks(mod, kind):
    """The forward pre-hooks of `mod` where it can be taken apart -- exactly a `kind` (no subclass) without forward hooks or
    parametrizations, whose only pre-hooks are the legacy torch.nn.utils.spectral_norm's (it recomputes .weight from weight_orig / u / v and
    returns nothing) -- else None"""
    pre = list(mod._forward_pre_hooks.values())
    if type(mod) is kind and not mod._forward_hooks and not getattr(mod, "parametrizations", None) and all(isinstance(h, SpectralNorm) for h in pre):
        return pre
    return None


def _plain_conv_weight(conv, x):
    """The weight of `conv` as its forward would use it on `x`, for callers that take the convolution apart -- or None when that
    is not safe.  Only a plain Conv2d, or one whose single extra is the legacy torch.nn.utils.spectral_norm pre-hook, is taken apart;
    anything else -- forward hooks, the parametrizations API, a pre-hook that edits the input, another padding mode -- goes through
    Module.__call__ untouched."""
    pre = _sn_hooks(conv, nn.Conv2d)
    if pre is None or conv.padding_mode != "zeros":
        return None
    return _normalised_weight(conv, pre, x)


def _normalised_weight(mod, pre, x):
    """mod.weight as mod's spectral-norm pre-hooks leave it.  In eval mode the hook does no power iteration -- weight_orig / sigma with
    sigma from the stored u, v is a constant of the checkpoint, yet torch recomputes it at every forward (a matrix-vector product, a
    dot and a division: ~270 launches of a few microseconds per decoder pass, a tenth of its time once the convolutions are
    fast).  Here it is computed once and kept until weight_orig / u / v change (their storage or version counters).  In train() or grad
    mode: the weight spectral_train.normalise left pending on `mod`, taken once and assigned to mod.weight as the hook would; with
    nothing pending, the hook."""
    if not pre:
        return mod.weight

    def hooked():
        for hook in pre:
            hook(mod, (x,))
        return mod.weight
    if mod.training or torch.is_grad_enabled():
        weight = take_pending(mod)
        if weight is None:
            return hooked()
        mod.weight = weight
        return weight
    return cached(mod, "_ps_sn_cache", (mod.weight_orig, mod.weight_u, mod.weight_v), lambda: hooked().detach())


def _sn_linear(lin, x):
    """lin(x) for the bias-free, possibly spectral-normalised Linear layers of LinearNoiseLayer, the normalised weight cached as above."""
    pre = _sn_hooks(lin, nn.Linear)
    if pre is None or lin.bias is not None:
        return lin(x)
    return F.linear(x, _normalised_weight(lin, pre, x))


_MIOPEN_SAFE_BYTES = 2 ** 31


def _conv2d_batches(fn, x, out_channels, stride=1):
    """fn(x) -- a convolution through torch (MIOpen) -- with the batch cut so that neither the input nor the output of a call
    reaches 2 GiB: MIOpen's fp32 NHWC kernels index with 32 bits, and a (128, 128, 256, 256) activation -- 4 GiB, the decoder's
    widest layer at C5's 128 views -- comes back WRONG, silently (8e-2 of the output's scale against an fp64 convolution,
    tools/conv_f16x3_big_check.py; at 64 views, 2 GiB, it is right).  The split-fp16 kernel indexes frames with 64 bits."""
    B = x.size(0)
    per = max(x[0].numel(), out_channels * (x.size(2) // stride) * (x.size(3) // stride)) * x.element_size()
    n = max(1, min(B, (_MIOPEN_SAFE_BYTES - 1) // max(per, 1)))
    if not x.is_cuda or n >= B:
        return fn(x)
    return torch.cat([fn(x[i:i + n]) for i in range(0, B, n)])


def conv1x1(conv, x):
    """conv(x) WITHOUT the bias for a 1 x 1 convolution (stride 1, no padding) on a channels-last CUDA fp32 activation, through
    csrc/conv1x1.hip (fp32 matrix pipe: exact fp32 products) -- or None when `conv` / `x` are not that (the caller goes through torch)."""
    if not (plain_conv(conv, 1, 0) and gpu_f32(x, multiple=4) and not torch.is_grad_enabled()):
        return None
    Ci, Co = conv.in_channels, conv.out_channels
    if not _lib.call("ps_conv1x1_takes", Ci, Co):
        return None
    weight = _plain_conv_weight(conv, x)
    if weight is None or weight.dtype != torch.float32 or not weight.is_cuda or weight.device != x.device:
        return None
    w2 = cached(conv, "_ps_1x1_cache", (weight,), lambda: weight.detach().reshape(Co, Ci).contiguous())
    B, _, H, W = x.shape
    y = empty_nhwc(B, Co, H, W, x)
    _lib.call("ps_conv1x1_nhwc_f32", x, w2, B * H * W, Ci, Co, y)
    return y


def _conv_split(conv, x, mode=None, opt=None):
    """conv(x) as (output WITHOUT the bias, bias) on the inference GPU path -- torch adds a convolution's bias in a pass
    of its own; here the per-channel constant rides along in whatever pass consumes the output (csrc/nets.hip).  Elsewhere
    (CPU, autograd, channel counts the kernels do not take): (conv(x), None).  mode "f16x3": a 1 x 1 convolution through
    csrc/conv1x1.hip instead of torch (MIOpen).  In grad mode with the training opt-in of `opt` (f16x3.train_mode) a wide 3 x 3
    convolution goes through f16x3.conv3x3_train (_f16x3_train_conv), and with the block opt-in (block_train.mode) a wide 1 x 1
    convolution through block_train.conv1x1_train (_block_train_conv1x1), and with the thin opt-in (thin_train.mode) the thin 3 x 3 and
    1 x 1 convolutions at the decoder's ends through thin_train's Functions (_thin_train_conv)."""
    if mode == "f16x3":
        y = conv1x1(conv, x)
        if y is not None:
            return y, conv.bias
    y = _f16x3_train_conv(conv, x, opt)
    if y is not None:
        return y, None
    y = _block_train_conv1x1(conv, x, opt)
    if y is not None:
        return y, None
    y = _thin_train_conv(conv, x, opt)
    if y is not None:
        return y, None
    if has_pending(conv):       # (its normalised weight is there already: conv(x) would run the hook's power iteration a second time)
        weight = _plain_conv_weight(conv, x)
        if weight is not None:
            return _conv2d_batches(lambda t: F.conv2d(t, weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups), x,
                                   conv.out_channels, conv.stride[0]), None
    if conv.bias is None or torch.is_grad_enabled() or not gpu_f32(x, multiple=4) or conv.out_channels % 4:
        return _conv2d_batches(conv, x, conv.out_channels, conv.stride[0]), None
    weight = _plain_conv_weight(conv, x)
    if weight is None:
        return _conv2d_batches(conv, x, conv.out_channels, conv.stride[0]), None
    return _conv2d_batches(lambda t: F.conv2d(t, weight, None, conv.stride, conv.padding, conv.dilation, conv.groups), x,
                           conv.out_channels, conv.stride[0]), conv.bias


# ---- the training routes: conv(x) WITH its bias as a torch.autograd.Function whose passes are HIP kernels --------------------------------
def _train_route(conv, x, opt, switch, want, k, pad, takes, run):
    """run(x channels-last, weight, conv.bias), or None: only in grad mode, only under the route's opt-in (switch.resolve(opt) == want),
    not where decoder_conv("fp32") or the options send the decoder's convolutions through torch, and only for a plain k x k convolution
    on a CUDA fp32 input (in any storage: it is made channels-last here) whose sizes takes(Ci, Co) accepts.  The weight is the module's own
    (with spectral norm: as its pre-hook leaves it, which is differentiable in training mode)."""
    if not (torch.is_grad_enabled() and switch.resolve(opt) == want and _conv_mode(opt) == "f16x3" and plain_conv(conv, k, pad)
            and gpu_f32(x, layout=None) and takes(conv.in_channels, conv.out_channels)):
        return None
    weight = _plain_conv_weight(conv, x)
    if weight is None or weight.dtype != torch.float32 or weight.device != x.device:
        return None
    # (what torch's norm + ReLU in front hands over usually is channels-last already)
    return run(x.contiguous(memory_format=torch.channels_last), weight, conv.bias)


def _f16x3_train_conv(conv, x, opt=None):
    """conv(x) through f16x3.conv3x3_train -- forward and backward pass on the fp16 matrix pipe -- or None (_train_route): the opt-in is
    decoder_conv_train("f16x3") / opt.decoder_conv_train / PS_DECODER_CONV_TRAIN (the default is "fp32"), the sizes those _f16x3_takes
    would take without autograd whose Ci is a multiple of 64 as well.  The weight is packed at every call: training weights change every
    step."""
    def run(x, weight, bias):
        try:
            return f16x3.conv3x3_train(x, weight, bias)
        except ValueError:      # a weight fp16 cannot hold: torch, on the weight already normalised (the pre-hook has run once)
            return F.conv2d(x, weight, bias, 1, 1)
    return _train_route(conv, x, opt, f16x3.decoder_conv_train, "f16x3", 3, 1,
                        lambda Ci, Co: f16x3.train_takes(Ci, Co, x.size(2), x.size(3)), run)


def _block_train_conv1x1(conv, x, opt=None):
    """conv(x) through block_train.conv1x1_train -- csrc/conv1x1.hip forward, csrc/block_train.hip and conv1x1.hip backward -- or None
    (_train_route): the opt-in is decoder_block_train("hip") / opt.decoder_block_train / PS_DECODER_BLOCK_TRAIN (the default is "torch"),
    the sizes Ci and Co multiples of 64 up to 256 (the projections of the decoder's four resampling blocks) and a multiple of 16 pixels."""
    return _train_route(conv, x, opt, block_train.decoder_block_train, "hip", 1, 0,
                        lambda Ci, Co: (Ci % 64 == 0 and Co % 64 == 0 and max(Ci, Co) <= block_train.MAX_CHANNELS
                                        and block_train.conv1x1_takes(Ci, Co, x.size(0) * x.size(2) * x.size(3))),
                        block_train.conv1x1_train)


def _thin_train_conv(conv, x, opt=None):
    """conv(x) through thin_train.conv_thin_in_train (4 -> Co) or conv_thin_out_train (Ci -> at most 4 channels) -- csrc/conv_thin.hip or
    conv1x1.hip forward, those and csrc/thin_train.hip backward -- or None (_train_route): the opt-in is decoder_thin_train("hip") /
    opt.decoder_thin_train / PS_DECODER_THIN_TRAIN (the default is "torch"), the convolution 3 x 3 or 1 x 1, the sizes
    thin_train.takes_in / takes_out (the decoder's block 0 and block 7)."""
    k = getattr(conv, "kernel_size", (0,))[0]
    if k not in (1, 3):
        return None
    thin_in = conv.in_channels == thin_train.THIN_IN
    takes = thin_train.takes_in if thin_in else thin_train.takes_out
    return _train_route(conv, x, opt, thin_train.decoder_thin_train, "hip", k, k // 2,
                        lambda Ci, Co: takes(Ci, Co, k, x.size(2), x.size(3)),
                        thin_train.conv_thin_in_train if thin_in else thin_train.conv_thin_out_train)


def _unet_train_conv(conv, x):
    """conv(x) WITH its bias for a 3 x 3 convolution of the depth Unet's way up, or None: only in grad mode under unet_train("hip") --
    that switch alone, not decoder_conv_train or decoder_thin_train -- with the decoder's convolutions on "f16x3" (_conv_mode), for a
    plain 3 x 3 convolution on a CUDA fp32 input: through f16x3.conv3x3_train where f16x3.train_takes holds (dconv4..6 of Unet(32) at
    256 x 256), through thin_train.conv_thin_out_train where thin_train.takes_out holds (dconv8).  The weight is the module's own as
    Unet._conv takes it: a pending spectral_train result, else the hook's.  A weight fp16 cannot hold, or anything else the Functions
    refuse: torch, on the weight already normalised."""
    if not (torch.is_grad_enabled() and unet_train.mode() == "hip" and _conv_mode() == "f16x3" and plain_conv(conv, 3, 1)
            and gpu_f32(x, layout=None)):
        return None
    Ci, Co, H, W = conv.in_channels, conv.out_channels, x.size(2), x.size(3)
    if f16x3.train_takes(Ci, Co, H, W):
        run = f16x3.conv3x3_train
    elif thin_train.takes_out(Ci, Co, 3, H, W):
        run = thin_train.conv_thin_out_train
    else:
        return None
    weight = _plain_conv_weight(conv, x)
    if weight is None or weight.dtype != torch.float32 or weight.device != x.device:
        return None
    x = x.contiguous(memory_format=torch.channels_last)
    try:
        return run(x, weight, conv.bias)
    except ValueError:
        return F.conv2d(x, weight, conv.bias, 1, 1)


# ---- the no-grad 3 x 3 routes ------------------------------------------------------------------------------------------------------------
def _thin_conv(conv, x, scale=None, shift=None):
    """conv(act(x)) WITHOUT the bias for the decoder's two thin 3 x 3 layers (4 -> Co, Ci -> <= 4 channels) through csrc/conv_thin.hip
    (fp32 FMAs), or None when `conv` is not one of them."""
    Ci, Co = conv.in_channels, conv.out_channels
    thin_in, thin_out = Ci == 4 and Co % 4 == 0 and Co <= 256, Ci % 32 == 0 and 1 <= Co <= 4
    if not (plain_conv(conv, 3, 1) and (thin_in or thin_out) and gpu_f32(x)
            and ((thin_in and Co == 64 and x.size(3) % 16 == 0) or (x.size(2) % 8 == 0 and x.size(3) % (64 if thin_in else 32) == 0))
            and not torch.is_grad_enabled()):
        return None
    weight = _plain_conv_weight(conv, x)
    if weight is None:
        return None
    wl = cached(conv, "_ps_thin_cache", (weight,), lambda: weight.detach().permute(2, 3, 1, 0).contiguous())      # [ky][kx][ci][co]
    if thin_in and Co == 64 and x.size(3) % 16 == 0:   # on the fp16 matrix pipe (split operands): 82 instead of 270 us per 16 views
        return f16x3.conv3x3_thin_in(x, wl, scale, shift)
    B, _, H, W = x.shape
    y = empty_nhwc(B, Co, H, W, x)
    if thin_in:
        _lib.call("ps_conv3x3_thin_in_nhwc_f32", x, scale, shift, wl, B, H, W, Co, y)
    else:
        _lib.call("ps_conv3x3_thin_out_nhwc_f32", x, scale, shift, wl, B, H, W, Ci, Co, y)
    return y


def _f16x3_takes(conv, x):
    return (plain_conv(conv, 3, 1) and conv.in_channels % 32 == 0 and conv.out_channels % 64 == 0 and gpu_f32(x, multiple=4)
            and x.size(2) % 16 == 0 and x.size(3) % 16 == 0 and x.size(2) * x.size(3) * x.size(1) < 2 ** 31 and not torch.is_grad_enabled())


def _f16x3_conv(conv, x, scale=None, shift=None, bias=None, res=None):
    """conv(act(x)) WITHOUT the convolution's own bias through the split-fp16 kernel (f16x3.conv3x3), act = max(x * scale - shift, 0)
    with scale / shift (B, C) contiguous, or the identity; `bias` (Co) and `res` (an NHWC tensor of the output's shape) are added on the
    way out.  None when the kernel does not take this convolution (the caller then goes through torch)."""
    if not _f16x3_takes(conv, x):
        return None
    weight = _plain_conv_weight(conv, x)
    if weight is None:
        return None

    def pack():
        try:
            return f16x3.pack3x3(weight.detach())
        except ValueError:                   # a weight fp16 cannot hold: this layer stays on torch
            return None
    packed = cached(conv, "_ps_f16x3_cache", (weight,), pack)     # once per weight (with spectral norm in eval mode: per checkpoint, see _normalised_weight)
    if packed is None or (res is not None and not (gpu_f32(res, multiple=4) and res.shape == (x.size(0), conv.out_channels) + x.shape[2:])):
        return None
    return f16x3.conv3x3(x, packed, scale, shift, bias, res)


# ---- the join of a block's two branches --------------------------------------------------------------------------------------------------
def _resample_sum(kind, a, b, bias=None, post=None, opt=None):
    """_resample(kind, a + bias) + _resample(kind, b) -- blocks.py:61-73 -- as ONE pass through csrc/nets.hip on the GPU
    (`bias`: per-channel constant still missing from the inputs, see _conv_split).  b = None: a alone -- resampling is linear, so
    a caller that already holds the SUM of the two branches resamples once.  post ('Down' only): a tensor of the output's shape added
    after the pooling.  Where autograd follows an operand: through block_train.resample_sum_train under its opt-in (block_train.mode(opt)
    "hip"; `bias` and `post` None, which they are in grad mode), else through torch."""
    # (an operand that autograd follows goes through torch: the HIP passes are forward-only and would cut the graph)
    graph = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (a, b, bias, post))
    if graph and bias is None and post is None and block_train.mode(opt) == "hip" and block_train.resample_takes(kind, a, b):
        return block_train.resample_sum_train(kind, a, b)
    if (graph or not gpu_f32(a, multiple=4) or (b is not None and not (gpu_f32(b, multiple=4) and a.shape == b.shape))
            or (kind and kind != "Up" and (a.size(2) % 2 or a.size(3) % 2)) or (b is None and not kind)):
        if bias is not None:
            a = a + bias.view(1, -1, 1, 1)
        out = _resample(kind, a) if b is None else _resample(kind, a) + _resample(kind, b)
        return out if post is None else out + post
    B, C, H, W = a.shape
    if not kind:
        out = torch.empty_like(a)
        _lib.call("ps_add_bias_nhwc_f32", a, b, bias, B, H * W, C, out)
    elif kind == "Up":
        out = empty_nhwc(B, C, 2 * H, 2 * W, a)
        _lib.call("ps_upsample_add_nhwc_f32", a, b, bias, B, H, W, C, out)
    else:
        out = empty_nhwc(B, C, H // 2, W // 2, a)
        if post is not None and not (gpu_f32(post, multiple=4) and post.shape == out.shape):
            raise ValueError("_resample_sum: post must be a channels_last tensor of the pooled shape")
        _lib.call("ps_pool_add_post_nhwc_f32", a, b, bias, post, B, H, W, C, out)
        return out
    if post is not None:
        raise ValueError("_resample_sum: post goes with 'Down' only")
    return out


def _resample(kind, x):
    if kind == "Up":
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    if kind:            # "Down" or True
        return F.avg_pool2d(x, kernel_size=3, stride=2, padding=1)
    return x
