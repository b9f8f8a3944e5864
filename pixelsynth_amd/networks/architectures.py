"""The dense networks either side of the hot path: the depth regressor `Unet`
(models/networks/architectures.py:174-279) and the refinement `ResNetDecoder` (:126-167) with its blocks
(models/layers/blocks.py:34-73) and noise-conditioned normalisation (models/layers/normalization.py:21-47, :97-200).

Same constructor arguments, attribute / parameter names and shapes as the reference, so its checkpoints load with
`load_state_dict(strict=True)`; the bodies are written for inference on one MI355X:

  * NHWC (channels_last) on the GPU; inputs are converted on entry, results handed back NCHW-contiguous because the HIP kernels
    downstream take raw NCHW pointers;
  * the DECODER's 3 x 3 convolutions are hand-written (csrc/conv_f16x3.hip through f16x3.py, which also owns its overflow guard: split-fp16
    MFMA, fp32 in / out, the norm + ReLU in front applied as the input is staged; csrc/conv_thin.hip for the 4 -> 64 and 128 -> 3 layers): 8.3 instead of 20 ms
    per 16 views; its 1 x 1 projections run on the fp32 matrix pipe (csrc/conv1x1.hip, round 6).  PS_DECODER_CONV=fp32 /
    opt.decoder_conv = "fp32" sends them through torch.  The Unet's convolutions and the decoder's 3 -> 3 layer run through torch (MIOpen), the batch cut so that no call sees 2 GiB (MIOpen's fp32 NHWC
    kernels are silently wrong on 4 GiB activations -- 128 views of the decoder's widest layer);
  * spectral-normalised weights are computed once per checkpoint in eval mode, not at every forward (_normalised_weight);
  * `LinearNoiseLayer` + stored-statistics batch norm + ReLU is ONE per-(sample, channel) affine and a clamp
    (`_noise_affine`), not four elementwise passes;
  * `ResNetDecoder.forward(..., noise=)` takes the noise draws explicitly (a list of (B,20) tensors, two per block) so
    a run is reproducible and comparable with the reference; without it the draws come from torch.randn as there.

Training: the plain BatchNorm2d layers are torch's own.  The noise-conditioned layers in train() normalise on batch statistics and
update the stored ones (the running average, or standing sums with bn.accumulate_standing) through norm_train.batch_norm_train:
csrc/norm_train.hip -- statistics, norm + ReLU and their backward pass -- for channels-last fp32 activations on the GPU, the torch formula
elsewhere or under decoder_norm_train("torch").  In eval() every path is the stored-statistics form above, untouched.  Under
decoder_block_train("hip") (block_train.py; the default is "torch") a block's wide 1 x 1 projection and its Up / Down join are
differentiated by csrc/block_train.hip as well, and under decoder_thin_train("hip") (thin_train.py; the default is "torch") the thin
first and last layers -- block 0's 4 -> 64 and block 7's 128 -> 3 convolutions, 3 x 3 and 1 x 1 -- by csrc/thin_train.hip.

This file holds what a checkpoint sees and the blocks' dataflow.  Which kernel a convolution or a join gets is decided in conv_routes.py;
the five route switches and the test of what the kernels accept as a tensor are routing.py's.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from . import conv_routes, norm_train, spectral_train, unet_train
from .block_train import decoder_block_train  # noqa: F401
from .norm_train import decoder_norm_train  # noqa: F401
from .thin_train import decoder_thin_train  # noqa: F401
from .f16x3 import check_f16x3_overflow, decoder_conv, decoder_conv_train  # noqa: F401  (the names bench.py and the tests use)
# The routes are looked up in THIS module's namespace when a block runs: the tests replace _f16x3_conv here with a spy, and bench.py and
# tools/ reach them as arch.<name>.
from .conv_routes import (_conv2d_batches, _conv_mode, _conv_split, _f16x3_conv, _f16x3_takes, _f16x3_train_conv,  # noqa: F401
                          _normalised_weight, _overflow_flag, _plain_conv_weight, _resample, _resample_sum, _sn_hooks, _sn_linear,
                          _thin_conv, conv1x1, plain_conv)
from .routing import empty_nhwc, gpu_f32, has_pending, per_sample
from .vgg19 import VGG19  # noqa: F401  (the content loss's network, where the reference keeps it)

NOISE_SZ = 20
# "f16x3" | "fp32" (everything through torch / MIOpen): the process default of decoder_conv, read at every call (bench.py assigns it)
DECODER_CONV = decoder_conv.from_env()

# decoder tables of get_resnet_arch (models/networks/configs.py): first width, then (width, resample) per block.
_DEC_WIDTHS = lambda g: [g, 2 * g, 4 * g, 4 * g, 2 * g, 2 * g, 2 * g, 3]
_DEC_RESAMPLE = [None, "Down", "Down", None, "Up", "Up", None, None]
_DEC_FIRST = {"256W8UpDown": lambda c: 128, "256W8UpDown64": lambda c: 64, "256W8UpDownDV": lambda c: 64,
              "256W8UpDownRGB": lambda c: 3, "256W8UpDown3": lambda c: c, "256W8UpDown3SuperRes": lambda c: c}


def _spectral(opt):
    return "spectral" in opt.norm_G


def _conv(opt, cin, cout, k, stride, pad):
    conv = nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad)
    return nn.utils.spectral_norm(conv) if _spectral(opt) else conv


def _norm_layer(opt):
    kind = opt.norm_G.split(":")[1]
    if kind in ("batch", "spectral_batch"):
        return nn.BatchNorm2d
    if kind == "spectral_instance":
        return nn.InstanceNorm2d
    if kind == "spectral_batchstanding":
        return BatchNorm_StandingStats
    raise ValueError("unknown norm_G %r" % opt.norm_G)


class bn(nn.Module):
    """The BigGAN-style batch norm (normalization.py:117-166); buffers only.  eval(): the stored statistics; train(): the batch's, the
    stored ones updated (networks/norm_train.py)."""

    def __init__(self, num_channels, eps=1e-5, momentum=0.1):
        super().__init__()
        self.eps, self.momentum, self.accumulate_standing = eps, momentum, False
        self.register_buffer("stored_mean", torch.zeros(num_channels))
        self.register_buffer("stored_var", torch.ones(num_channels))
        self.register_buffer("accumulation_counter", torch.zeros(1))

    def reset_stats(self):
        """Zero the standing statistics and their counter (before accumulate_standing passes)"""
        with torch.no_grad():
            self.stored_mean.zero_()
            self.stored_var.zero_()
            self.accumulation_counter.zero_()

    def scale_shift(self, gain, bias, x=None, pend=None):
        """y = x * scale - shift with gain/bias (B or 1, C, 1, 1) folded in (fused_bn, normalization.py:170-184).  In training mode the
        statistics are those of the activation `x` (through torch; the stored ones move, `pend` -- a bias still missing from x -- going
        into the stored mean), so x must be given."""
        if self.training:
            if x is None:
                raise RuntimeError("noise-conditioned batch norm in training mode: the batch statistics need the activation, scale_shift(gain, bias, x)")
            mean, var = norm_train.batch_stats(x, self, pend)
        else:
            mean, var = self.stored_mean.view(1, -1, 1, 1), self.stored_var.view(1, -1, 1, 1)
            if self.accumulate_standing:
                mean, var = mean / self.accumulation_counter, var / self.accumulation_counter
        scale = torch.rsqrt(var + self.eps) * gain
        return scale, mean * scale - bias

    def forward(self, x, gain, bias):
        if self.training:
            return norm_train.batch_norm_train(x, gain, bias, self, relu=False)
        scale, shift = self.scale_shift(gain, bias)
        return x * scale - shift


class BatchNorm_StandingStats(nn.Module):
    def __init__(self, output_size, eps=1e-5, momentum=0.1):
        super().__init__()
        self.output_size, self.eps, self.momentum = output_size, eps, momentum
        self.gain = nn.Parameter(torch.ones(output_size))
        self.bias = nn.Parameter(torch.zeros(output_size))
        self.bn = bn(output_size, eps, momentum)

    def forward(self, x, y=None):
        return self.bn(x, self.gain.view(1, -1, 1, 1), self.bias.view(1, -1, 1, 1))


class LinearNoiseLayer(nn.Module):
    """Gain and bias of a batch norm predicted from a noise vector (normalization.py:21-47)."""

    def __init__(self, opt, noise_sz=NOISE_SZ, output_sz=32):
        super().__init__()
        self.noise_sz = noise_sz
        lin = lambda: nn.Linear(noise_sz, output_sz, bias=False)
        self.gain = nn.utils.spectral_norm(lin()) if _spectral(opt) else lin()
        self.bias = nn.utils.spectral_norm(lin()) if _spectral(opt) else lin()
        self.bn = bn(output_sz)

    def gain_bias(self, x, noise=None):
        """The gain and bias (B, C, 1, 1) this layer predicts from `noise` (drawn here when None); through torch, differentiable"""
        if noise is None:
            noise = torch.randn(x.size(0), self.noise_sz).to(x.device)
        B = noise.size(0)
        return (1 + _sn_linear(self.gain, noise)).view(B, -1, 1, 1), _sn_linear(self.bias, noise).view(B, -1, 1, 1)

    def affine(self, x, noise=None, pend=None):
        """(scale, shift) of the layer on x; in training mode from x's batch statistics (bn.scale_shift), where `pend` is a bias still
        missing from x"""
        gain, bias = self.gain_bias(x, noise)
        return self.bn.scale_shift(gain, bias, x, pend) if self.bn.training else self.bn.scale_shift(gain, bias)

    def affine_bc(self, x, noise=None, pend=None):
        """affine() as contiguous (B, C) scale / shift -- what the HIP passes take -- with `pend` (C), a convolution bias still missing
        from x, folded into shift.  On the inference GPU path ONE launch (ps_noise_affine_f32) instead of two matrix products and six
        elementwise kernels; elsewhere composed from affine()."""
        if noise is None:
            noise = torch.randn(x.size(0), self.noise_sz).to(x.device)
        B, C = noise.size(0), self.bn.stored_mean.numel()
        bufs = (self.bn.stored_mean, self.bn.stored_var)
        if (x.is_cuda and not torch.is_grad_enabled() and not self.training and not self.bn.accumulate_standing and B == x.size(0)
                and noise.dtype == torch.float32 and noise.is_cuda and noise.device == x.device   # (the kernel takes raw pointers: a host
                # tensor or one of another device must go the torch way, where it raises the usual device-mismatch error)
                and all(t.is_cuda and t.device == x.device and t.dtype == torch.float32 and t.is_contiguous() for t in bufs)
                and (pend is None or (pend.is_cuda and pend.device == x.device and pend.dtype == torch.float32 and pend.is_contiguous()))
                and self.gain.bias is None and self.bias.bias is None):
            ws = []
            for lin in (self.gain, self.bias):
                pre = _sn_hooks(lin, nn.Linear)
                if pre is None:
                    ws = None
                    break
                ws.append(_normalised_weight(lin, pre, noise).contiguous())
            if ws is not None:
                noise = noise.contiguous()
                scale = torch.empty(B, C, dtype=torch.float32, device=x.device)
                shift = torch.empty_like(scale)
                _lib.call("ps_noise_affine_f32", noise, ws[0], ws[1], self.bn.stored_mean, self.bn.stored_var, pend, float(self.bn.eps), B, C,
                          noise.size(1), scale, shift)
                return scale, shift
        scale, shift = self.affine(x, noise, pend)
        if pend is not None and not self.bn.training:     # (on batch statistics a constant missing from x cancels: nothing to fold)
            shift = shift - pend.view(1, -1, 1, 1) * scale
        Bx = x.size(0)
        return per_sample(scale, Bx, C), per_sample(shift, Bx, C)

    def forward(self, x, noise=None):
        if self.bn.training:
            return self.bn(x, *self.gain_bias(x, noise))
        scale, shift = self.affine(x, noise)
        return x * scale - shift


class _Slots(nn.Module):
    """Sub-modules registered under the indices the reference's nn.Sequential gave them (checkpoint key names)."""

    def __init__(self, **at):
        super().__init__()
        for idx, mod in at.items():
            self.add_module(idx.lstrip("_"), mod)

    def __getitem__(self, idx):
        return self._modules[str(idx)]


def _nhwc(module, x):
    """On the GPU: weights (once) and input to channels_last."""
    if not x.is_cuda:
        return x
    if not getattr(module, "_nhwc_ready", False):
        module.to(memory_format=torch.channels_last)
        module._nhwc_ready = True
    return x.contiguous(memory_format=torch.channels_last)


def _sum_bias(*bs):
    bs = [b for b in bs if b is not None]
    return None if not bs else bs[0] if len(bs) == 1 else (bs[0] + bs[1]).contiguous()


def _on_batch_stats(layer):
    """Whether `layer` is a LinearNoiseLayer whose batch norm is in training mode (anything else a caller hands in has an affine() alone)"""
    return hasattr(layer, "gain_bias") and layer.bn.training


class ResNet_Block(nn.Module):
    """(norm, relu, 3x3) x 2 (+ resample) on one branch, 1x1 (+ resample) or identity on the other (blocks.py:34-73)."""

    def __init__(self, in_c, in_o, opt, downsample=None):
        super().__init__()
        self.opt = opt
        self.resample = downsample
        self.ch_a = _Slots(_0=LinearNoiseLayer(opt, output_sz=in_c), _2=_conv(opt, in_c, in_o, 3, 1, 1),
                           _3=LinearNoiseLayer(opt, output_sz=in_o), _5=_conv(opt, in_o, in_o, 3, 1, 1))
        self.projected = bool(downsample) or in_c != in_o
        if self.projected:
            self.ch_b = _Slots(_0=_conv(opt, in_c, in_o, 1, 1, 0))

    @staticmethod
    def _noise_affine(layer, x, noise, bias=None, affine=None):
        """norm + ReLU of (x + bias): y = max(x * scale[b][c] - shift[b][c], 0), a pending conv bias folded into shift --
        one HIP pass on the GPU (ps_affine_relu_nhwc_f32).  A layer in training mode: on the batch statistics of x, the stored ones
        updated (norm_train.batch_norm_train; the bias then only shifts the stored mean)."""
        if affine is None and _on_batch_stats(layer):
            gain, offset = layer.gain_bias(x, noise)
            if x.is_cuda:      # (what the convolution or resampling in front hands over usually is already)
                x = x.contiguous(memory_format=torch.channels_last)
            return norm_train.batch_norm_train(x, gain, offset, layer.bn, True, bias)
        if affine is None and gpu_f32(x, multiple=4) and not torch.is_grad_enabled() and hasattr(layer, "affine_bc"):
            affine = layer.affine_bc(x, noise, bias)
        if affine is not None:   # (bias already folded in; as (B, C) or broadcastable to (B, C, 1, 1))
            scale, shift = (t.view(t.size(0), -1, 1, 1) if t.dim() == 2 else t for t in affine)
        else:
            scale, shift = layer.affine(x, noise)
            if bias is not None:
                shift = shift - bias.view(1, -1, 1, 1) * scale
        B, C = x.size(0), x.size(1)
        if gpu_f32(x, multiple=4) and scale.numel() in (C, B * C) and not torch.is_grad_enabled():
            y = torch.empty_like(x)   # (preserves channels_last)
            _lib.call("ps_affine_relu_nhwc_f32", x, per_sample(scale, B, C), per_sample(shift, B, C), B, x.size(2) * x.size(3), C, y)
            return y
        return torch.clamp_min(torch.addcmul(-shift, x, scale), 0)

    def _norm_relu_conv(self, layer, conv, x, noise, bias=None, res=None, out_bias=None):
        """conv(relu(norm(x + bias))) as (output without the convolution's own bias, that bias, fused).  The decoder's 3 x 3 layers:
        ONE kernel, norm + ReLU applied as the patch is staged (csrc/conv_f16x3.hip, conv_thin.hip); the others: the affine pass, then
        torch.  res / out_bias: the block's other branch and the biases still pending, which the split-fp16 kernel adds on its way out
        (`fused` says whether it did: the output is then conv + res + out_bias)."""
        mode = _conv_mode(self.opt)
        if _on_batch_stats(layer):
            # batch statistics: the norm + ReLU is a pass of its own (norm_train); without autograd -- how standing statistics are
            # collected -- the decoder's own convolutions follow with the identity in front
            y = self._noise_affine(layer, x, noise, bias)
            if mode == "f16x3" and conv.bias is not None and y.is_cuda and not torch.is_grad_enabled():
                out = _f16x3_conv(conv, y) if _f16x3_takes(conv, y) else _thin_conv(conv, y)
                if out is not None:
                    return out, conv.bias, False
            return _conv_split(conv, y, opt=self.opt) + (False,)
        if mode == "f16x3" and conv.bias is not None and x.is_cuda and not torch.is_grad_enabled():
            scale, shift = layer.affine_bc(x, noise, bias)
            if _f16x3_takes(conv, x):
                y = _f16x3_conv(conv, x, scale, shift, out_bias, res)
                if y is not None:
                    return y, conv.bias, res is not None or out_bias is not None
                y = _f16x3_conv(conv, x, scale, shift)
            else:
                y = _thin_conv(conv, x, scale, shift)
            if y is not None:
                return y, conv.bias, False
            return _conv_split(conv, self._noise_affine(layer, x, None, None, affine=(scale, shift))) + (False,)
        return _conv_split(conv, self._noise_affine(layer, x, noise, bias), opt=self.opt) + (False,)

    def forward(self, x, noise=(None, None)):
        a, ba, _ = self._norm_relu_conv(self.ch_a[0], self.ch_a[2], x, noise[0])
        mode = _conv_mode(self.opt)
        # (not in train(): the test of the 1 x 1 weight below would run its spectral norm's power iteration a second time)
        if (self.resample and self.resample != "Up" and mode == "f16x3" and gpu_f32(x, multiple=4) and not torch.is_grad_enabled() and not self.training
                and x.size(2) % 2 == 0 and x.size(3) % 2 == 0 and plain_conv(self.ch_b[0], 1, 0)
                # (the 1 x 1 conv's bias must come back SEPARATE from _conv_split, to go through the pool's bias * inside / 9 term: a
                # convolution that cannot be taken apart returns conv(x) + bias, whose border pixels would then differ from the reference's)
                and (self.ch_b[0].bias is None or (self.ch_b[0].out_channels % 4 == 0 and _plain_conv_weight(self.ch_b[0], x) is not None))):
            # Down: avg_pool2d and the 1 x 1 convolution of the other branch commute -- pool first, convolve a quarter of the pixels,
            # and hand the result to the pooling of this branch as its `post` term (both biases ride through the pooling: bias=)
            b, bb = _conv_split(self.ch_b[0], _resample_sum(self.resample, x, None), mode)
            a, ba2, _ = self._norm_relu_conv(self.ch_a[3], self.ch_a[5], a, noise[1], ba)
            return _resample_sum(self.resample, a, None, _sum_bias(ba2, bb), post=b)
        b, bb = _conv_split(self.ch_b[0], x, mode, self.opt) if self.projected else (x, None)
        # The second convolution adds the other branch on its way out where it can (resampling is linear: resample(a) + resample(b) =
        # resample(a + b)); without resampling the biases go in as well and its output is the block's.
        conv2 = self.ch_a[5]
        own = conv2.bias if conv2.bias is not None and not self.resample else None
        a, ba2, fused = self._norm_relu_conv(self.ch_a[3], conv2, a, noise[1], ba, res=b,
                                             out_bias=None if self.resample else _sum_bias(own, bb))
        if fused:
            return a if not self.resample else _resample_sum(self.resample, a, None, _sum_bias(ba2, bb), opt=self.opt)
        return _resample_sum(self.resample if self.projected else None, a, b, _sum_bias(ba2, bb), opt=self.opt)


class ResNetDecoder(nn.Module):
    """The refinement network (architectures.py:126-167): eight blocks, tanh, optional residual around them."""

    def __init__(self, opt, channels_in=64, channels_out=3, use_tanh=True):
        super().__init__()
        self.opt = opt
        setup = opt.refine_model_type.split("_")[1]
        if setup not in _DEC_FIRST:
            raise ValueError("refine_model_type %r: decoder table not built" % opt.refine_model_type)
        widths = [_DEC_FIRST[setup](channels_in)] + _DEC_WIDTHS(opt.ngf)
        self.eblocks = nn.ModuleList([ResNet_Block(widths[i], widths[i + 1], opt, _DEC_RESAMPLE[i]) for i in range(8)])
        if use_tanh:
            self.norm = nn.Tanh()

    def n_noise(self):
        return 2 * len(self.eblocks)

    def forward(self, x, background_mask=None, noise=None):
        if (background_mask is not None and gpu_f32(x, layout=torch.contiguous_format) and x.size(1) == 3
                and background_mask.dtype == torch.bool and background_mask.is_contiguous()
                and background_mask.shape == (x.size(0), x.size(2), x.size(3)) and not torch.is_grad_enabled()):
            B, _, H, W = x.shape
            h = empty_nhwc(B, 4, H, W, x)          # cat + NCHW -> NHWC in one pass
            _lib.call("ps_cat_mask_nhwc_f32", x, background_mask, B, H, W, h)
            _nhwc(self, h)                            # (the weights, once)
        else:
            h = x if background_mask is None else torch.cat((x, (~background_mask).unsqueeze(1).float()), 1)
            h = _nhwc(self, h)
        if h.is_cuda and spectral_train.active(self, self.opt):
            # the 22 convolutions and 32 noise linears in one batched pass; each takes its weight where it asks for it (_normalised_weight)
            spectral_train.normalise(spectral_train.sn_modules(self), self.opt)
        if noise is None and h.is_cuda:
            # the reference draws each layer's noise on the host and sends it over (normalization.py:36-37): sixteen small blocking
            # copies per pass.  The same sixteen draws, in the same order from the same generator, in ONE copy.
            noise = torch.stack([torch.randn(h.size(0), NOISE_SZ) for _ in range(self.n_noise())]).to(h.device).unbind(0)
        for i, blk in enumerate(self.eblocks):
            h = blk(h, (None, None) if noise is None else (noise[2 * i], noise[2 * i + 1]))
        if getattr(self.opt, "predict_residual", False):
            if background_mask is not None and getattr(self.opt, "normalize_before_residual", False):
                return (self.norm(h) + x).contiguous()
            return self.norm(h + x).contiguous()
        return self.norm(h).contiguous()


class Unet(nn.Module):
    """Depth regressor (architectures.py:174-279): 8 stride-2 4x4 convolutions down to 1x1, 8 x (bilinear x2, 3x3)
    back up with skip concatenations; leaky ReLU on the way down, ReLU on the way up, no norm on conv1 / conv8 / dconv8."""

    _ENC_NORM = [None, "batch_norm2_0", "batch_norm4_0", "batch_norm8_0", "batch_norm8_1", "batch_norm8_2", "batch_norm8_3", None]
    _DEC_NORM = ["batch_norm8_4", "batch_norm8_5", "batch_norm8_6", "batch_norm8_7", "batch_norm4_1", "batch_norm2_1", "batch_norm", None]

    def __init__(self, num_filters=32, channels_in=3, channels_out=3, use_tanh=False, use_3D=False, opt=None):
        super().__init__()
        if use_3D:
            raise NotImplementedError("3-D Unet is not part of the novel-view path")
        f = num_filters
        enc = [channels_in, f, 2 * f, 4 * f, 8 * f, 8 * f, 8 * f, 8 * f, 8 * f]
        dec_out = [8 * f, 8 * f, 8 * f, 8 * f, 4 * f, 2 * f, f, channels_out]
        norm = _norm_layer(opt)
        for i in range(8):
            setattr(self, f"conv{i + 1}", _conv(opt, enc[i], enc[i + 1], 4, 2, 1))
            if self._ENC_NORM[i]:
                setattr(self, self._ENC_NORM[i], norm(enc[i + 1]))
        for i in range(8):
            cin = enc[8] if i == 0 else dec_out[i - 1] + enc[8 - i]          # previous output ++ the mirrored encoder level
            setattr(self, f"dconv{i + 1}", _conv(opt, cin, dec_out[i], 3, 1, 1))
            if self._DEC_NORM[i]:
                setattr(self, self._DEC_NORM[i], norm(dec_out[i]))

    MAX_BATCH = 64   # images per call on the GPU, at most

    def _images_per_call(self, H, W):
        """dconv8 reads 2 f channels at the input's size: the call's batch keeps that activation below the 2 GiB at which MIOpen's fp32
        kernels start to index wrongly (_conv2d_batches) -- by bytes, so at 512 x 512 it is a quarter of what it is at 256 x 256."""
        per = self.dconv8.in_channels * H * W * 4
        return max(1, min(self.MAX_BATCH, (conv_routes._MIOPEN_SAFE_BYTES - 1) // per))

    @staticmethod
    def _conv(conv, x):
        """conv(x); in eval mode without autograd with the spectral-normalised weight computed once per checkpoint (_normalised_weight)
        instead of at every forward -- torch's hook costs five small launches per layer, a fifth of this network's time at 8 images; and
        with the weight spectral_train.normalise left pending at the top of forward() instead of the hook's."""
        if has_pending(conv) or (x.is_cuda and not torch.is_grad_enabled() and not conv.training):
            weight = _plain_conv_weight(conv, x)
            if weight is not None:
                return F.conv2d(x, weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups)
        return conv(x)

    def forward(self, input):
        if input.is_cuda and not torch.is_grad_enabled() and not self.training:
            n = self._images_per_call(input.size(2), input.size(3))
            if input.size(0) > n:
                return torch.cat([self.forward(input[i:i + n]) for i in range(0, input.size(0), n)])
        skips, h = [], _nhwc(self, input)
        if h.is_cuda and spectral_train.active(self):      # (this network keeps no options: the switch's block, or PS_SPECTRAL_TRAIN)
            spectral_train.normalise(spectral_train.sn_modules(self))
        if unet_train.active(self, h):
            return self._forward_hip(h)
        for i in range(8):
            h = self._conv(getattr(self, f"conv{i + 1}"), h if i == 0 else F.leaky_relu(h, 0.2))
            if self._ENC_NORM[i]:
                h = getattr(self, self._ENC_NORM[i])(h)
            skips.append(h)
        for i in range(8):
            if h.size(2) == 1 and h.size(3) == 1 and h.is_cuda:
                # bilinear x 2 of a single pixel is that pixel four times (torch takes its NCHW kernel for a 1 x 1 map: 0.26 ms of the
                # network's 1.7 per 8 images)
                h = F.relu(h).expand(-1, -1, 2, 2).contiguous(memory_format=torch.channels_last)
            else:
                h = F.interpolate(F.relu(h), scale_factor=2, mode="bilinear", align_corners=False)
            h = self._conv(getattr(self, f"dconv{i + 1}"), h)
            if self._DEC_NORM[i]:
                h = torch.cat((getattr(self, self._DEC_NORM[i])(h), skips[6 - i]), 1)
        return h.contiguous()

    def _forward_hip(self, h):
        """The loop of forward() under unet_train("hip") (networks/unet_train.py): a norm and the leaky ReLU behind it in one pass, the
        skip tensor and the tensor beside it never concatenated -- relu and the bilinear x2 read both where they lie --, the wide 3 x 3
        convolutions through conv_routes._unet_train_conv.  Each piece hands what it does not take to the expression of forward().  What a
        convolution hands on is made channels-last where it is not (torch's own kernels, with the library's switched off, answer in
        NCHW): no copy otherwise."""
        nhwc = lambda t: t.contiguous(memory_format=torch.channels_last)
        skips, act = [], h
        for i in range(8):
            h = nhwc(self._conv(getattr(self, f"conv{i + 1}"), act))
            if self._ENC_NORM[i]:
                h, act = unet_train.bn_act_train(h, getattr(self, self._ENC_NORM[i]), 0.2)
            elif i < 7:
                act = F.leaky_relu(h, 0.2)
            skips.append(h)
        a, b = h, None
        for i in range(8):
            h = unet_train.relu_up2_cat(a, b)
            conv = getattr(self, f"dconv{i + 1}")
            y = conv_routes._unet_train_conv(conv, h)
            h = nhwc(self._conv(conv, h)) if y is None else y
            if self._DEC_NORM[i]:
                a, b = unet_train.bn_act_train(h, getattr(self, self._DEC_NORM[i])), skips[6 - i]
        return h.contiguous()


def get_decoder(opt):
    """models/networks/utilities.py:26-36 for the resnet decoders (the mask channel is there unless no_outpainting)."""
    if "resnet" not in opt.refine_model_type:
        raise ValueError("refine_model_type %r: only the resnet decoders are built" % opt.refine_model_type)
    return ResNetDecoder(opt, channels_in=3 + (0 if getattr(opt, "no_outpainting", False) else 1), channels_out=3)
