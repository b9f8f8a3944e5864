"""The likelihood the PixelCNN gives to GIVEN codes (csrc/code_nll.hip behind include/pixelsynth_nll.h): what the reference reports on
every validation pass -- autoreg_loss = CrossEntropyLoss()(outpaint2(one_hot(gt_codes), masks), gt_codes), models/z_buffermodel.py:351-381
and :398; train_lmconv.py:406 and :584-587 report the same quantity in bits -- on the device; without gradients from the fused engine
(score_codes), and as a loss to differentiate from the layer-by-layer network (ar_loss).

    code_nll      logits + target codes -> per location nll, entropy, hit; per frame their fp64 sums per group (observed / sampled)
    score_codes   ONE whole-grid forward of the engine on the given codes with a plan's masks, then code_nll: the masks made from an
                  order admit only predecessors and mask_init is type A, so one pass gives every conditional at once
    ar_loss       the same mean cross entropy as a differentiable loss: OurPixelCNN's layers on the one-hot codes, every masked convolution
                  and its backward a HIP kernel (csrc/lmconv_bwd.hip) -- what train_lmconv.py minimises

Nothing comes down to the host: every field of the result is a device tensor, and so is what its methods return.
"""
import math

import torch

from . import _lib
from .ar_plan import ARPlan
from .lmconv.locally_masked_convolution import compact_mask

CLASSES = 512
LAYOUTS = ("chw", "lc")                 # (F,512,L) / (F,512,H,W): PixelCNNEngine.forward; (F,L,512): out_logits of the AR runs
GROUPS = ("all", "sampled", "observed")
COUNT, NLL, ENTROPY, HIT = range(4)     # the columns of CodeNLL.frames


class CodeNLL:
    """nll, entropy (F,L) fp32 in nats; hit (F,L) uint8; frames (F,2,4) fp64: [f][g] = count, sum nll, sum entropy, sum hit over the
    locations of group g, 0 = observed, 1 = sampled.  The methods are the means over the frames' locations of a group ("all",
    "sampled", "observed") as 0-dim fp64 tensors where `frames` is -- (F,) per frame with per_frame=True; a group without a location
    has no mean: NaN."""

    def __init__(self, nll, entropy, hit, frames, temperature=1.0):
        self.nll, self.entropy, self.hit, self.frames, self.temperature = nll, entropy, hit, frames, float(temperature)

    def sums(self, group="all", per_frame=False):
        """The four columns of `frames` summed over the group's rows (and over the frames) -> (4,) fp64, or (F,4)"""
        if group not in GROUPS:
            raise ValueError(f"group is {group!r}, expected one of {GROUPS}")
        rows = self.frames.sum(1) if group == "all" else self.frames[:, 1 if group == "sampled" else 0]
        return rows if per_frame else rows.sum(0)

    def _mean(self, column, group, per_frame, scale=1.0):
        s = self.sums(group, per_frame)
        return s[..., column] / s[..., COUNT] * scale

    def mean_nll(self, group="all", per_frame=False):
        """Nats per code: what nn.CrossEntropyLoss() returns for the group's locations (at temperature 1)"""
        return self._mean(NLL, group, per_frame)

    def bits_per_code(self, group="all", per_frame=False):
        """mean_nll / ln 2 (train_lmconv.py:584)"""
        return self._mean(NLL, group, per_frame, 1.0 / math.log(2.0))

    def mean_entropy_bits(self, group="all", per_frame=False):
        return self._mean(ENTROPY, group, per_frame, 1.0 / math.log(2.0))

    def accuracy(self, group="all", per_frame=False):
        """The share of the group's locations whose target is the arg-max of the logits"""
        return self._mean(HIT, group, per_frame)


def code_nll(logits, targets, region=None, temperature=1.0, layout="chw"):
    """logits fp32 on the device, (F,512,L) or (F,512,H,W) for layout "chw", (F,L,512) for "lc"; targets (F,L) or (F,H,W) integer codes;
    region (F,L) or (F,H,W), nonzero = sampled, None: every location observed -> CodeNLL (asynchronous on the current stream).
    A NaN logit gives a NaN nll there and in its group's sum; a target outside [0, 512) gives a NaN nll and hit 0."""
    if layout not in LAYOUTS:
        raise ValueError(f"code_nll: layout is {layout!r}, expected one of {LAYOUTS}")
    if not temperature > 0:
        raise ValueError(f"code_nll: temperature = {temperature}, expected > 0")
    _lib.require_cuda(logits, targets, region)
    if logits.dtype != torch.float32:
        raise ValueError(f"code_nll: logits are {logits.dtype}, expected torch.float32")
    F_ = logits.shape[0]
    if layout == "chw":
        ok, L = logits.dim() in (3, 4) and logits.shape[1] == CLASSES, logits[0, 0].numel() if logits.dim() in (3, 4) else 0
    else:
        ok, L = logits.dim() == 3 and logits.shape[2] == CLASSES, logits.shape[1] if logits.dim() == 3 else 0
    if not ok or F_ < 1 or L < 1:
        raise ValueError(f"code_nll: logits of shape {tuple(logits.shape)} for layout {layout!r}: expected "
                         + ("(F,512,L) or (F,512,H,W)" if layout == "chw" else "(F,L,512)"))
    if targets.shape[0] != F_ or targets.numel() != F_ * L:
        raise ValueError(f"code_nll: targets of shape {tuple(targets.shape)} for {F_} frames of {L} locations")
    if region is not None and (region.shape[0] != F_ or region.numel() != F_ * L):
        raise ValueError(f"code_nll: region of shape {tuple(region.shape)} for {F_} frames of {L} locations")
    dev = logits.device
    logits = logits.contiguous()
    targets = targets.reshape(F_, L).to(torch.int32).contiguous()
    if region is not None:
        region = (region.reshape(F_, L) != 0).to(torch.uint8).contiguous() if region.dtype != torch.uint8 else region.reshape(F_, L).contiguous()
    nll, entropy = (torch.empty(F_, L, dtype=torch.float32, device=dev) for _ in range(2))
    hit = torch.empty(F_, L, dtype=torch.uint8, device=dev)
    frames = torch.empty(F_, 2, 4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("ps_code_nll_f32", logits, LAYOUTS.index(layout), targets, region, float(temperature), F_, L, nll, entropy, hit, frames)
    return CodeNLL(nll, entropy, hit, frames, temperature)


def _engine_of(model_or_engine, H, W, F_):
    """ZbufferModelPts (its outpaint2), OurPixelCNN (its engine for F_ frames) or a PixelCNNEngine -> the engine"""
    net = getattr(model_or_engine, "outpaint2", model_or_engine)
    if hasattr(net, "engine"):
        return net.engine(H, W, F_)
    if not hasattr(net, "handle"):
        raise TypeError(f"score_codes: {type(model_or_engine).__name__} is neither a model with a PixelCNN engine nor an engine")
    if (net.H, net.W) != (H, W):
        raise ValueError(f"score_codes: an engine of a {net.H} x {net.W} grid for codes of a {H} x {W} one")
    return net


def _plan_args(who, codes, plan_or_masks, region):
    """-> (H, W, the three masks one copy per frame, region) of the arguments score_codes and ar_loss share"""
    F_ = codes.shape[0]
    if isinstance(plan_or_masks, ARPlan):
        plan = plan_or_masks
        H, W = plan.H, plan.W
        masks = (plan.mask_init, plan.mask_undilated, plan.mask_dilated)
        if region is None:
            region = plan.region
    else:
        if len(plan_or_masks) != 3:
            raise ValueError(f"{who}: an ARPlan or the three masks (mask_init, mask_undilated, mask_dilated) expected")
        if codes.dim() != 3:
            raise ValueError(f"{who}: with masks the codes carry the grid, (F,H,W); got {tuple(codes.shape)}")
        H, W = codes.shape[1:]
        masks = tuple(compact_mask(m.to(codes.device), F_, c) for m, c in zip(plan_or_masks, (CLASSES + 1, 160, 80)))
    if codes.numel() != F_ * H * W:
        raise ValueError(f"{who}: codes of shape {tuple(codes.shape)} for a {H} x {W} grid")
    _lib.require_cuda(codes)
    return H, W, masks, region


def score_codes(model_or_engine, codes, plan_or_masks, region=None, temperature=1.0):
    """The likelihood of `codes` (F,H,W) -- or (F,L) with a plan, whose grid it is -- under the PixelCNN in the generation order of
    `plan_or_masks`: the compact ARPlan, or the three masks (mask_init, mask_undilated, mask_dilated) as get_masks_for_batch returns them
    -- (F*513,9,L), (F*160,9,L), (F*80,9,L) -- or one copy per frame, (F|1,9,L).  One PixelCNNEngine.forward on the codes (every
    location's logits are conditioned on its predecessors' codes alone), then code_nll on its logits.  region: None takes the plan's
    sampled region (every location observed where only masks are given) -> CodeNLL."""
    F_ = codes.shape[0]
    H, W, masks, region = _plan_args("score_codes", codes, plan_or_masks, region)
    with torch.cuda.device(codes.device):
        logits = _engine_of(model_or_engine, H, W, F_).forward(codes, *masks)
    return code_nll(logits, codes, region, temperature, "chw")


def ar_loss(model, codes, plan_or_masks, region=None, group="sampled", temperature=1.0):
    """The mean cross entropy in nats of `codes` over the locations of `group` ("all", "sampled", "observed") as a DIFFERENTIABLE 0-dim
    fp32 loss -- the quantity score_codes(...).mean_nll(group) reports from the fused engine, here from OurPixelCNN._forward_layers on
    the one-hot codes: plain torch but for the masked convolutions, whose forward and backward are HIP kernels -- or, under
    pixelcnn_train("hip") (lmconv/train_ops.py: the block, opt.pixelcnn_train of a model with options, PS_PIXELCNN_TRAIN; default "torch"), with
    the normalisations, activations, gates and the loss's backward on HIP as well.  Arguments as
    score_codes; model: ZbufferModelPts (its outpaint2) or OurPixelCNN.  After optimizer.step() the model's engine rebuilds itself
    (it is keyed on the parameters' versions), so sampling and scoring use the tuned weights.  A group without a location: NaN."""
    if group not in GROUPS:
        raise ValueError(f"ar_loss: group is {group!r}, expected one of {GROUPS}")
    if not temperature > 0:
        raise ValueError(f"ar_loss: temperature = {temperature}, expected > 0")
    net = getattr(model, "outpaint2", model)
    if not hasattr(net, "_forward_layers"):
        raise TypeError(f"ar_loss: {type(model).__name__} is not a model with the PixelCNN's layers (an engine holds no parameters to tune)")
    F_ = codes.shape[0]
    H, W, masks, region = _plan_args("ar_loss", codes, plan_or_masks, region)
    targets = codes.reshape(F_, H * W).long()
    x = torch.nn.functional.one_hot(targets.view(F_, H, W), CLASSES).permute(0, 3, 1, 2).float()
    from .lmconv import train_ops
    if train_ops.mode(getattr(model, "opt", None)) == "hip":
        # the layers' passes between the convolutions and the loss's backward on csrc/pixelcnn_train.hip; the logits stay in the (F,H,W,512)
        # storage nin_out leaves them in, and the value is sum nll / count of code_nll's fp64 sums: score_codes(...).mean_nll(group)'s formula
        with train_ops.pixelcnn_train("hip"), torch.cuda.device(codes.device):
            return train_ops.code_cross_entropy(net._forward_layers(x, True, *masks), targets, region, group, temperature)
    with train_ops.pixelcnn_train("torch"), torch.cuda.device(codes.device):
        logits = net._forward_layers(x, True, *masks).reshape(F_, CLASSES, H * W)
        nll = torch.nn.functional.cross_entropy(logits / float(temperature), targets, reduction="none")
        if group == "all":
            return nll.mean()
        sampled = torch.zeros_like(nll, dtype=torch.bool) if region is None else region.reshape(F_, H * W) != 0
        take = sampled if group == "sampled" else ~sampled
        return torch.where(take, nll, torch.zeros_like(nll)).sum() / take.sum()
