"""What the PixelCNN's training pass runs between its masked convolutions (the reference's models/lmconv/layers.py gated_resnet and
PONO, models/lmconv/utils.py concat_elu, and the CrossEntropyLoss of train_lmconv.py):

norm_act(x, skip=None, norm=True, act="celu" | "elu" | None)   act(PONO(x) [+ skip]) of an NCHW activation; "celu" doubles the channels
gate(vg, u)                                                    u + PONO(v) * sigmoid(g), (v, g) the two halves of vg along the channels
code_cross_entropy(logits, targets, region, group, T)          the mean cross entropy of given codes over a group's locations, 0-dim fp32

Two routes each:

  "hip"    csrc/pixelcnn_train.hip (libpixelsynth_pixelcnn_train.so) as torch.autograd.Functions, once differentiable: one launch
           forward and one backward per call, fp64 sums over a location's channels, the same bits from run to run and at any
           place of a batch.  Saved for the backward pass: the operands and two statistics per location, never an intermediate.  For
           CUDA fp32 dense NCHW tensors (skip and the logits: dense NCHW or the dense (B,H,W,C) storage behind nin's movedim view;
           their gradients come back in the same storage, nothing is copied).
  "torch"  the torch formula, autograd's own backward -- the expressions of layers.py, literally: the CPU, fp64, C = 1, other storages
           -- and everything under pixelcnn_train("torch").

The switch: pixelcnn_train(...) in effect, else opt.pixelcnn_train, else PS_PIXELCNN_TRAIN, else the default below.
"""
import torch
import torch.nn.functional as F

from .. import _lib
from ..networks.routing import Switch, gpu_f32
from .utils import concat_elu

pixelcnn_train = Switch("pixelcnn_train", "PS_PIXELCNN_TRAIN", ("hip", "torch"), "torch", __name__, "PIXELCNN_TRAIN", attr="pixelcnn_train")
PIXELCNN_TRAIN = pixelcnn_train.from_env()   # "torch" (the layers as they were) | "hip" (the Functions below, where they take the tensors)
mode = pixelcnn_train.resolve                # the route in effect

ACTS = (None, "elu", "celu")                 # PS_PCT_ACT_* of include/pixelsynth_pixelcnn_train.h
NCHW, NHWC = 0, 1                            # PS_PCT_NCHW, PS_PCT_NHWC
MAX_CHANNELS = 65536                         # PS_PCT_MAX_CHANNELS
CLASSES = 512
GROUP_BITS = {"observed": 1, "sampled": 2, "all": 3}   # PS_PCT_GROUP_*


def lanes_per_location(locations):
    """Lanes a launch over this many locations gives each of them (4 or 1): a function of B * H * W alone"""
    return _lib.call("ps_pixelcnn_train_lanes", int(locations))


# ------------------------------------------------------------------------------------------------------------------ the torch route
def pono_formula(x, epsilon=1e-5):
    var, mean = torch.var_mean(x, dim=1, keepdim=True, unbiased=True)
    return (x - mean) / torch.sqrt(var + epsilon)


def norm_act_formula(x, skip=None, norm=True, act="celu"):
    z = pono_formula(x) if norm else x
    if skip is not None:
        z = z + skip
    return concat_elu(z) if act == "celu" else F.elu(z) if act == "elu" else z


def gate_formula(vg, u):
    value, gate_ = vg.chunk(2, dim=1)
    return u + pono_formula(value) * torch.sigmoid(gate_)


def cross_entropy_formula(logits, targets, region=None, group="all", temperature=1.0):
    """logits (F,512,H,W) or (F,512,L), targets (F,L) int64 -> the mean over the group's locations, as likelihood.ar_loss writes it"""
    F_ = logits.shape[0]
    nll = F.cross_entropy(logits.reshape(F_, logits.shape[1], -1) / float(temperature), targets.reshape(F_, -1).long(), reduction="none")
    if group == "all":
        return nll.mean()
    sampled = torch.zeros_like(nll, dtype=torch.bool) if region is None else region.reshape(F_, -1) != 0
    take = sampled if group == "sampled" else ~sampled
    return torch.where(take, nll, torch.zeros_like(nll)).sum() / take.sum()


# -------------------------------------------------------------------------------------------------------------------- the HIP route
def _storage(t):
    """NCHW / NHWC for a tensor dense as it is / with its channels (dimension 1) last, else None"""
    if t.is_contiguous():
        return NCHW
    return NHWC if t.movedim(1, -1).is_contiguous() else None


def takes(x, norm=True):
    """What the kernels take as their main operand: CUDA fp32 (B,C,H,W) dense NCHW, not empty, C >= 2 where PONO runs, B H W < 2^31"""
    return (gpu_f32(x, layout=torch.contiguous_format) and x.numel() > 0 and (2 if norm else 1) <= x.size(1) <= MAX_CHANNELS
            and x.size(0) * x.size(2) * x.size(3) < 2 ** 31)


def _empty_like_storage(t, storage):
    """An uninitialised tensor of t's shape in t's dense storage"""
    if storage == NCHW:
        return torch.empty_like(t, memory_format=torch.contiguous_format)
    return torch.empty_like(t.movedim(1, -1), memory_format=torch.contiguous_format).movedim(-1, 1)


class _NormAct(torch.autograd.Function):
    """x (B,C,H,W) dense NCHW fp32, skip None or of x's shape in `storage`.  Saves x, skip, mean and rstd (one each per location); the
    normalised value, z and the activation's branch are recomputed."""

    @staticmethod
    def forward(ctx, x, skip, norm, act, storage):
        B, C, H, W = x.shape
        y = torch.empty(B, 2 * C if act == 2 else C, H, W, dtype=torch.float32, device=x.device)
        mean, rstd = (torch.empty(B * H * W, dtype=torch.float32, device=x.device) for _ in range(2)) if norm else (None, None)
        with torch.cuda.device(x.device):
            _lib.call("ps_norm_act_forward_f32", x, skip, storage, B, C, H * W, int(norm), act, y, mean, rstd)
        ctx.save_for_backward(x, skip, mean, rstd)
        ctx.norm, ctx.act, ctx.storage = norm, act, storage
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, skip, mean, rstd = ctx.saved_tensors
        B, C, H, W = x.shape
        need_x, need_skip = ctx.needs_input_grad[0], skip is not None and ctx.needs_input_grad[1]
        if not (need_x or need_skip):
            return None, None, None, None, None
        dy = grad_y.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if need_x else None
        dskip = _empty_like_storage(skip, ctx.storage) if need_skip else None
        with torch.cuda.device(x.device):
            _lib.call("ps_norm_act_backward_f32", x, skip, ctx.storage, dy, mean, rstd, B, C, H * W, int(ctx.norm), ctx.act, dx, dskip)
        return dx, dskip, None, None, None


class _Gate(torch.autograd.Function):
    """vg (B,2C,H,W), u (B,C,H,W) dense NCHW fp32.  Saves vg, mean and rstd; u's gradient is the incoming one itself."""

    @staticmethod
    def forward(ctx, vg, u):
        B, C, H, W = u.shape
        out = torch.empty_like(u)
        mean, rstd = (torch.empty(B * H * W, dtype=torch.float32, device=u.device) for _ in range(2))
        with torch.cuda.device(u.device):
            _lib.call("ps_gate_forward_f32", vg, u, B, C, H * W, out, mean, rstd)
        ctx.save_for_backward(vg, mean, rstd)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        vg, mean, rstd = ctx.saved_tensors
        B, C2, H, W = vg.shape
        dvg = None
        if ctx.needs_input_grad[0]:
            dout = grad_out.to(torch.float32).contiguous()
            dvg = torch.empty_like(vg)
            with torch.cuda.device(vg.device):
                _lib.call("ps_gate_backward_f32", vg, dout, mean, rstd, B, C2 // 2, H * W, dvg)
        return dvg, grad_out if ctx.needs_input_grad[1] else None


class _CodeCrossEntropy(torch.autograd.Function):
    """logits (F,512,H,W) or (F,512,L) fp32 in `storage`; the forward is likelihood.code_nll (ps_code_nll_f32) on them as they lie, the
    value sum nll / count of its fp64 `frames`; saves the logits, targets, region and `frames`."""

    @staticmethod
    def forward(ctx, logits, targets, region, group, temperature, storage):
        from ..likelihood import COUNT, NLL, code_nll
        F_ = logits.shape[0]
        rows = logits if storage == NCHW else logits.movedim(1, -1).reshape(F_, -1, CLASSES)      # (views: nothing is copied)
        score = code_nll(rows, targets, region, temperature, "chw" if storage == NCHW else "lc")
        ctx.save_for_backward(logits, targets, region, score.frames)
        ctx.group, ctx.temperature, ctx.storage = group, float(temperature), storage
        s = score.sums(group)
        return (s[NLL] / s[COUNT]).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        logits, targets, region, frames = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        F_, L = logits.shape[0], logits[0, 0].numel()
        grad = _empty_like_storage(logits, ctx.storage)
        go = grad_loss.to(torch.float32).reshape(1).contiguous()
        with torch.cuda.device(logits.device):
            _lib.call("ps_code_nll_backward_f32", logits, ctx.storage, targets, region, frames, GROUP_BITS[ctx.group], ctx.temperature,
                      F_, L, go, grad)
        return grad, None, None, None, None, None


# ------------------------------------------------------------------------------------------------------------------ the front ends
def norm_act(x, skip=None, norm=True, act="celu", opt=None):
    """act(PONO(x) [+ skip]): PONO the reference's (unbiased variance over the channels, eps 1e-5 inside the root), act the
    concatenated ELU ("celu": (B,2C,H,W), elu(z) then elu(-z)), "elu" or None.  Differentiable once in x and skip; works under
    torch.no_grad() too.  Module docstring: the routes."""
    if act not in ACTS:
        raise ValueError(f"norm_act: act is {act!r}, expected one of {ACTS}")
    if not norm and skip is None and act is None:
        return x
    if mode(opt) == "hip" and takes(x, norm):
        storage = NCHW if skip is None else _storage(skip) if gpu_f32(skip, layout=None) and skip.shape == x.shape else None
        if storage is not None:
            return _NormAct.apply(x, skip, bool(norm), ACTS.index(act), storage)
    return norm_act_formula(x, skip, norm, act)


def gate(vg, u, opt=None):
    """u + PONO(v) * sigmoid(g) with (v, g) = vg.chunk(2, 1): the last line of gated_resnet.forward"""
    if mode(opt) == "hip" and takes(u) and takes(vg) and vg.shape == (u.size(0), 2 * u.size(1), u.size(2), u.size(3)):
        return _Gate.apply(vg, u)
    return gate_formula(vg, u)


def code_cross_entropy(logits, targets, region=None, group="all", temperature=1.0, opt=None):
    """The mean over the locations of `group` ("all", "sampled", "observed") of the cross entropy in nats of softmax(logits / T) against
    `targets`: logits (F,512,H,W) or (F,512,L), targets (F,L) or (F,H,W) integer codes, region (F,L) or (F,H,W), nonzero = sampled, None:
    every location observed -> 0-dim fp32, the number likelihood.code_nll(...).mean_nll(group) reports.  A group without a location: NaN."""
    if group not in GROUP_BITS:
        raise ValueError(f"code_cross_entropy: group is {group!r}, expected one of {tuple(GROUP_BITS)}")
    if not temperature > 0:
        raise ValueError(f"code_cross_entropy: temperature = {temperature}, expected > 0")
    if (mode(opt) == "hip" and gpu_f32(logits, layout=None, dims=None) and logits.dim() in (3, 4) and logits.size(1) == CLASSES
            and logits.numel() > 0 and logits.size(0) <= 65535):
        storage = NCHW if logits.is_contiguous() else NHWC if logits.movedim(1, -1).is_contiguous() and logits.data_ptr() % 16 == 0 else None
        if storage is not None:
            F_ = logits.shape[0]
            t = targets.reshape(F_, -1).to(torch.int32).contiguous()
            r = None if region is None else (region.reshape(F_, -1) != 0).to(torch.uint8).contiguous()
            return _CodeCrossEntropy.apply(logits, t, r, group, float(temperature), storage)
    return cross_entropy_formula(logits, targets, region, group, temperature)
