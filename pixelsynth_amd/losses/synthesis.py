"""The generator's image loss, with the interface of the reference's models/losses/synthesis.py (SynthesisLoss, PerceptualLoss,
L1LossWrapper, PSNR, SSIM: the same names, arguments, dict keys and values), and content_loss, the VGG19 perceptual ("content") term as
one torch.autograd.Function on the HIP kernels.

content_loss(vgg, pred, gt) -> (total, levels):  levels (5,) = the batch mean of |relu*_1(pred) - relu*_1(gt)| at VGG19's five taps (what
nn.L1Loss takes), total = sum_l w_l levels[l], w = (1/32, 1/16, 1/8, 1/4, 1).  Differentiable once, in pred alone (through total; levels
carries no gradient).

The HIP route is taken when pred and gt are CUDA fp32 (P, 3, H, W) of any strides on one device, H and W multiples of 256 (the relu5_1
map must be a multiple of 16 for the convolution kernel), gt does not require grad, no parameter of vgg requires grad, the weights are on
that device and fp16 can hold them, and networks.f16x3.decoder_conv("fp32") is not in effect.  Anything else takes the torch formula
(torch_content_loss): the modules under autograd, on any device, the CPU included.

The HIP route, forward: the 2P images (prediction i is image i, its target image P + i) go through the network in one pass --
ps_content_input, conv1_1 (ps_conv3x3_thin_in_f16x3_nhwc) and its bias (ps_content_bias, added once), the other twelve convolutions
(ps_conv3x3_f16x3_ex_nhwc, the ReLU applied on the way in), ps_content_pool in front of conv2_1, conv3_1, conv4_1 and conv5_1,
ps_content_tap on the five tapped PRE-ReLU maps, ps_content_finish.  In grad mode the prediction's thirteen pre-ReLU maps are saved --
19 M floats, about 76 MB, per 256 x 256 image -- and the target's five tapped ones (8.5 MB); the target's other maps are dropped as they
are consumed.  Without grad nothing is saved.  Backward: ps_content_join seeds the gradient at conv5_1, then per convolution, last to
second, ps_conv3x3_bwd_prepare_f32 (the power-of-two scale), ps_conv3x3_f16x3_ex_nhwc on the flipped, transposed pack (an overflow word
of its own, never read: a gradient that is not finite is there to see in the result) -- f16x3.bwd_prepare and f16x3.grad_input, the
steps of f16x3.conv3x3_train's backward pass -- and ps_content_join (unscale, route through the
pool, add the tap's seed, mask by the ReLU); ps_conv3x3_thin_out_nhwc_f32 on conv1_1's flipped weight gives the image's gradient.
Nothing is read back and nothing synchronises.

The call is a guarded scope (f16x3.checked), decided here: an activation beyond fp16's range in either branch warns and the call is made
again through the torch formula.

The maps a call saved: content_loss(vgg, pred, gt, return_saved=True) -> (total, levels, saved), saved = {"maps": the thirteen (P, C, Hl,
Wl) channels_last pre-ReLU maps of the prediction (conv1_1's with its bias), "gt": the target's five tapped ones} -- the very tensors the
backward pass reads, not a second pass; None where the torch formula ran or nothing was saved.
"""
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _images, _lib
from ..networks import f16x3
from ..networks.routing import empty_nhwc
from ..networks.vgg19 import POOL_BEFORE, TAPPED, VGG19

WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)


def torch_content_loss(vgg, pred, gt):
    """The reference's formula (synthesis.py:94-104) through the modules, on any device -> (total, levels (5,) detached)"""
    gt_fs = vgg(gt)
    pred_fs = vgg(pred)
    loss, levels = 0, []
    for i in range(len(gt_fs)):
        level = F.l1_loss(pred_fs[i], gt_fs[i])
        loss += WEIGHTS[i] * level
        levels.append(level.detach())
    return loss, torch.stack(levels)


def hip_takes(vgg, pred, gt):
    """Whether content_loss(vgg, pred, gt) takes the HIP route (module docstring)"""
    if f16x3.forced_mode() == "fp32" or not hasattr(vgg, "hip_layers"):
        return False
    for t in (pred, gt):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.size(0) >= 1 and t.size(1) == 3
                and t.size(2) > 0 and t.size(3) > 0 and t.size(2) % 256 == 0 and t.size(3) % 256 == 0):
            return False
    if pred.shape != gt.shape or pred.device != gt.device or gt.requires_grad or any(p.requires_grad for p in vgg.parameters()):
        return False
    if pred.size(0) > 32767 or any(s < 0 for s in pred.stride() + gt.stride()):
        return False
    P, _, H, W = pred.shape
    if H * W * 64 >= 2 ** 31 or 2 * P * H * W > 2 ** 30:      # the convolution kernels' frame and batch (f16x3.train_takes; the 64-channel maps are the largest)
        return False
    dev = vgg.convs()[0].weight.device
    return dev == pred.device and all(c.weight.dtype == torch.float32 for c in vgg.convs()) and vgg.hip_layers(dev) is not None


def _network(layers, pred, gt, keep):
    """The forward pass -> (total (), levels (5,), saved or None)"""
    P, _, H, W = pred.shape
    dev, N = pred.device, 2 * pred.size(0)
    x = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
    _lib.call("ps_content_input", pred, _images.strides(pred), gt, _images.strides(gt), P, H, W, x)
    tiles = [_lib.call("ps_content_tiles", P * (H >> l) * (W >> l)) for l in range(5)]
    sums = torch.empty(sum(tiles), dtype=torch.float64, device=dev)
    counts, maps, gts, h = [], [], [], None
    for k in range(13):
        if k == 0:
            h = f16x3.conv3x3_thin_in(x.permute(0, 3, 1, 2), layers["w0"])
            _lib.call("ps_content_bias", h, layers["b0"], N * H * W, 64)
        else:
            if k in POOL_BEFORE:
                C, Hl, Wl = h.shape[1:]
                pooled = empty_nhwc(N, C, Hl // 2, Wl // 2, x)
                _lib.call("ps_content_pool", h, N, Hl, Wl, C, pooled)
                h = pooled
            p = layers["packed"][k - 1]
            h = f16x3.conv3x3(h, p, *f16x3.plain_relu(N, p["Ci"], dev))
        tapped = k in TAPPED
        if tapped:
            C, Hl, Wl = h.shape[1:]
            _lib.call("ps_content_tap", h, P, Hl, Wl, C, sums[sum(tiles[:len(counts)]):])
            counts.append(P * C * Hl * Wl)
        if keep:      # (a tapped map stays whole: its other half is the target's, which the backward pass reads too)
            maps.append(h[:P] if tapped else h[:P].clone(memory_format=torch.channels_last))
            if tapped:
                gts.append(h[P:])
    levels = torch.empty(5, dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.float32, device=dev)
    i64x5 = ctypes.c_int64 * 5
    _lib.call("ps_content_finish", sums, i64x5(*tiles), i64x5(*counts), levels, total)
    return total.reshape(()), levels, (dict(maps=maps, gt=gts) if keep else None)


def _join(y, y_gt, up, scale2, g, weight, pooled):
    P, C, Hl, Wl = y.shape
    G = torch.empty_like(y)          # (preserves channels_last)
    _lib.call("ps_content_join", y, y_gt, up, scale2, g if y_gt is not None else None, weight, P, Hl, Wl, C, int(pooled), G)
    return G


def _backward(layers, saved, g):
    """The gradient of total to pred (P, 3, H, W) for g = d loss / d total, a (1,) fp32 tensor on the device"""
    maps, gts = saved["maps"], saved["gt"]
    G = _join(maps[12], gts[4], None, None, g, WEIGHTS[4], False)
    for k in range(12, 0, -1):
        flipped = layers["flipped"][k - 1]
        gs, scale2, _, _ = f16x3.bwd_prepare(G, flipped["Co"])
        up = f16x3.grad_input(gs, flipped)          # still multiplied by the scale: the join divides
        level = TAPPED.index(k - 1) if k - 1 in TAPPED else None
        G = _join(maps[k - 1], None if level is None else gts[level], up, scale2, g, 0.0 if level is None else WEIGHTS[level],
                  k in POOL_BEFORE)
    P, _, H, W = G.shape
    gx = torch.empty((P, H, W, 3), dtype=torch.float32, device=g.device)
    _lib.call("ps_conv3x3_thin_out_nhwc_f32", G, None, None, layers["w0_flipped"], P, H, W, 64, 3, gx)
    return gx.permute(0, 3, 1, 2)


class _ContentLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, layers, holder, keep):
        total, levels, saved = _network(layers, pred.detach(), gt.detach(), keep)
        ctx.layers, ctx.saved = layers, saved      # (intermediates, neither inputs nor outputs: held by the graph node alone)
        ctx.mark_non_differentiable(levels)
        holder.append(saved)
        return total, levels

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, _g_levels):
        with torch.cuda.device(g_total.device):
            g = g_total.detach().to(torch.float32).reshape(1).contiguous()
            return _backward(ctx.layers, ctx.saved, g), None, None, None, None


def content_loss(vgg, pred, gt, return_saved=False):
    """The content term (module docstring) -> (total, levels), or (total, levels, saved) with return_saved"""
    holder = []
    if hip_takes(vgg, pred, gt):
        dev = pred.device
        # (decided here: inside a Function's forward grad mode always reads as off, and needs_input_grad does not know of no_grad)
        keep = torch.is_grad_enabled() and pred.requires_grad

        def run():
            del holder[:]
            if f16x3.forced_mode() == "fp32":      # the guard's rerun
                return torch_content_loss(vgg, pred, gt)
            with torch.cuda.device(dev):
                return _ContentLoss.apply(pred, gt, vgg.hip_layers(dev), holder, keep)
        total, levels = f16x3.checked(dev, run)
    else:
        total, levels = torch_content_loss(vgg, pred, gt)
    return (total, levels, holder[0] if holder else None) if return_saved else (total, levels)


class PerceptualLoss(nn.Module):
    """synthesis.py:85-104: the content term on a frozen VGG19.  The network's weights: `weights` (a path or a state dict) or
    opt.vgg19_weights, else torchvision's cached file; `rand` or opt.vgg19_rand: torchvision's initialisation (networks/vgg19.py, networks/vgg.py)."""

    def __init__(self, opt=None, weights=None, rand=None):
        super().__init__()
        weights = getattr(opt, "vgg19_weights", None) if weights is None else weights
        rand = bool(getattr(opt, "vgg19_rand", False)) if rand is None else rand
        self.model = VGG19(requires_grad=False, weights=weights, rand=rand)
        self.criterion = nn.L1Loss()
        self.weights = list(WEIGHTS)

    def forward(self, pred_img, gt_img):
        loss, _ = content_loss(self.model, pred_img, gt_img)
        return {"Perceptual": loss, "Total Loss": loss}


class L1LossWrapper(nn.Module):
    """synthesis.py:75-78"""

    def forward(self, pred_img, gt_img):
        err = F.l1_loss(pred_img, gt_img)
        return {"L1": err, "Total Loss": err}


class PSNR(nn.Module):
    """synthesis.py:60-66: 10 log10(1 / mse), the squared error summed over the channels and averaged over the pixels, then the batch
    mean; under no_grad."""

    def forward(self, pred_img, gt_img):
        with torch.no_grad():
            bs = pred_img.size(0)
            mse_err = (pred_img - gt_img).pow(2).sum(dim=1).view(bs, -1).mean(dim=1)
            return {"psnr": (10 * (1 / mse_err).log10()).mean()}


def _ssim_host(img1, img2):
    """The reference's SSIM (11-tap Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2) in torch, for tensors that
    are not on the ROCm device -> the mean of the SSIM map"""
    C = img1.size(1)
    taps = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)])
    taps = taps / taps.sum()
    window = torch.outer(taps, taps).to(img1).expand(C, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t, window, padding=5, groups=C)
    mu1, mu2 = blur(img1), blur(img2)
    s11, s22, s12 = blur(img1 * img1) - mu1 * mu1, blur(img2 * img2) - mu2 * mu2, blur(img1 * img2) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()


class SSIM(nn.Module):
    """synthesis.py:69-71, through losses.ssim.ssim (csrc/metrics.hip) for images on the device: forward only, so the value is
    detached; the kernel does not clamp, so it takes the [-1, 1] images as they come, as the reference's formula does.  Images that
    are not on the device go through the same formula in torch."""

    def forward(self, pred_img, gt_img):
        with torch.no_grad():
            if pred_img.is_cuda:
                from .ssim import ssim
                return {"ssim": ssim(pred_img.detach(), gt_img.detach())}
            return {"ssim": _ssim_host(pred_img.detach().float(), gt_img.detach().float())}


class SynthesisLoss(nn.Module):
    """synthesis.py:10-57.  opt.losses = ["<lambda>_<name>", ...] with names l1 and content; PSNR and SSIM are appended.  forward ->
    the union of the terms' dicts, "Total Loss" their combination with the reference's quirk kept: the first term's "Total Loss" is
    taken UNWEIGHTED and every later one is multiplied by its lambda (synthesis.py:46-53).  Not kept: the reference's
    get_loss_from_name returns None where there is no CUDA device; here it returns the module, moved to the device when there is one."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        lambdas, loss_names = zip(*[l.split("_") for l in opt.losses])
        self.lambdas = [float(l) for l in lambdas]
        loss_names += ("PSNR", "SSIM")
        self.losses = nn.ModuleList([self.get_loss_from_name(name) for name in loss_names])

    def get_loss_from_name(self, name):
        if name == "l1":
            loss = L1LossWrapper()
        elif name == "content":
            loss = PerceptualLoss(self.opt)
        elif name == "PSNR":
            loss = PSNR()
        elif name == "SSIM":
            loss = SSIM()
        else:
            raise ValueError(f"SynthesisLoss: unknown loss {name!r} (l1, content)")
        return loss.cuda() if torch.cuda.is_available() else loss

    def forward(self, pred_img, gt_img):
        out, total = {}, None
        for lam, term in zip(self.lambdas + [None, None], [loss(pred_img, gt_img) for loss in self.losses]):
            if "Total Loss" in term:
                total = term["Total Loss"] if total is None else total + term["Total Loss"] * lam
            for name, value in term.items():
                out.setdefault(name, value)      # (a name an earlier term gave stays)
        if total is not None:
            out["Total Loss"] = total
        return out
