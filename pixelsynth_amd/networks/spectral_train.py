"""Spectral normalisation in training as ONE batched pass per network forward (csrc/spectral_train.hip,
libpixelsynth_spectral_train.so) instead of torch's legacy torch.nn.utils.spectral_norm hook once per layer: the hook's training forward
is 38 aten ops per layer and its backward 18, two to three dozen launches of a few microseconds each, for 54 modules of the refinement
decoder, 16 of the Unet and 6 of the discriminator at every forward.

normalise(modules)   takes the modules it can -- a plain nn.Conv2d / nn.Linear on the GPU in fp32 whose only extra is the legacy hook
                     (name "weight", dim 0, one power iteration), and discriminators._SNConv -- through one torch.autograd.Function of
                     many outputs: all weight_orig in, all weight_orig / sigma out, the power iteration of the layers in training mode in
                     place on weight_u / weight_v as the hook does it.  Five launches forward and two backward for up to MAX_LAYERS
                     layers.  Each result is left PENDING on its module (routing.leave_pending);
the consumers        conv_routes._normalised_weight (before the hook) and _SNConv.weight() take a pending weight exactly once; with nothing
                     pending they do what they did.

Two routes: "hip", the above, at the top of ResNetDecoder.forward, Unet.forward and MultiscaleDiscriminator.forward in grad mode or in
train(); "torch", the hook, which is the default -- and what everything that normalise() does not take gets: the CPU, fp64, other hooks.
The switch: spectral_train(...) in effect, else opt.spectral_train, else PS_SPECTRAL_TRAIN.

Out of scope: n_power_iterations != 1, dim != 0 (transposed convolutions), the parametrizations API, double backward.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from .conv_routes import _sn_hooks
from .routing import Switch, leave_pending

spectral_train = Switch("spectral_train", "PS_SPECTRAL_TRAIN", ("hip", "torch"), "torch", __name__, "SPECTRAL_TRAIN", attr="spectral_train")
SPECTRAL_TRAIN = spectral_train.from_env()      # "hip" (normalise() at the top of a network's forward) | "torch" (the hook per layer)
mode = spectral_train.resolve                   # the route in effect
MAX_LAYERS = 64                                  # PS_SPECTRAL_MAX_LAYERS of include/pixelsynth_spectral_train.h: layers per call
PART_ROWS, TILE = 16, 4096                       # PS_SPECTRAL_PART_ROWS, PS_SPECTRAL_TILE
FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 5, 2       # PS_SPECTRAL_FORWARD_LAUNCHES, PS_SPECTRAL_BACKWARD_LAUNCHES
_WS = _lib.Workspace()
_TABLES = {}                                     # key of a table -> _Table; the addresses and sizes of a network do not change from step to step
_MAX_TABLES = 32


def active(module, opt=None):
    """Whether a network's forward runs normalise(): the "hip" route, and grad mode or train() -- never where the consumers would take the
    weight cached for eval mode without autograd"""
    return mode(opt) == "hip" and (torch.is_grad_enabled() or module.training)


def plan(R, C):
    """Host mirror of the library's plan for a layer of R x C: (parts of W^T u, groups of four rows, tiles)"""
    return (R + PART_ROWS - 1) // PART_ROWS, (R + 3) // 4, (R * C + TILE - 1) // TILE


def workspace_bytes(shapes):
    """Host mirror of ps_spectral_workspace_bytes for layers of the given (R, C): the parts of W^T u and a double per tile, the rows of
    s as doubles too, each region rounded up to 256 bytes"""
    up = lambda n: (n + 255) // 256 * 256
    parts, _, tiles = zip(*(plan(R, C) for R, C in shapes))
    return (up(8 * sum(p * C for p, (_, C) in zip(parts, shapes))) + up(8 * sum(tiles)) + up(8 * sum(R for R, _ in shapes)))


def _gpu_f32(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and len({t.device for t in tensors}) == 1


def _interleave(w):
    """How the columns of weight_orig (Co, ...) lie in memory (the header's `interleave`): 1 for a contiguous weight, Ci for a
    (Co, Ci, kh, kw) weight in channels-last storage -- what the networks here turn theirs into on the GPU --, None for any other"""
    if w.is_contiguous():
        return 1
    if w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last):
        return w.size(1)
    return None


def _layer(mod):
    """(weight_orig, u, v, iterates, eps, interleave) of a module normalise() takes, else None"""
    from .discriminators import _SNConv         # (it imports this module)
    if type(mod) is _SNConv:
        iterate, eps = mod.training and bool(getattr(mod.opt, "isTrain", False)), 1e-12
    elif type(mod) in (nn.Conv2d, nn.Linear):
        pre = _sn_hooks(mod, type(mod))
        if not pre or len(pre) != 1 or (pre[0].name, pre[0].dim, pre[0].n_power_iterations) != ("weight", 0, 1):
            return None
        if (mod.padding_mode != "zeros") if type(mod) is nn.Conv2d else (mod.bias is not None):     # (their callers go through the hook)
            return None
        if not (mod.training or torch.is_grad_enabled()):       # (the eval-mode cache of conv_routes._normalised_weight)
            return None
        iterate, eps = mod.training, float(pre[0].eps)
    else:
        return None
    w, u, v = mod.weight_orig, mod.weight_u, mod.weight_v
    inter = _interleave(w)
    if not (_gpu_f32(w, u, v) and inter and u.is_contiguous() and v.is_contiguous() and w.dim() >= 2 and w.numel() > 0 and eps > 0
            and u.numel() == w.size(0) and v.numel() == w.numel() // w.size(0)):
        return None
    return w, u, v, iterate, eps, inter


class _Table:
    """The library's table of some layers: its image in pinned host memory, its copy on the device (queued once, on the stream current
    then), the offsets of the flat buffers and the workspace's size"""

    def __init__(self, layers, device):
        n = len(layers)
        self.n, self.shapes = n, [(w.size(0), w.numel() // w.size(0)) for w, *_ in layers]
        ptrs = lambda i: (ctypes.c_void_p * n)(*[layer[i].data_ptr() for layer in layers])
        ints = lambda vals: (ctypes.c_int * n)(*vals)
        nbytes = _lib.call("ps_spectral_table_bytes")
        self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        offs = [(ctypes.c_longlong * (n + 1))() for _ in range(3)]
        _lib.call("ps_spectral_plan", ptrs(0), ptrs(1), ptrs(2), ints([R for R, _ in self.shapes]), ints([C for _, C in self.shapes]),
                  ints([layer[5] for layer in layers]), ints([int(layer[3]) for layer in layers]),
                  (ctypes.c_float * n)(*[layer[4] for layer in layers]), n, self.host.data_ptr(), nbytes, *offs)
        self.elem, self.row, self.col = (list(o) for o in offs)
        self.device = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.device.copy_(self.host, non_blocking=True)
        self.ws_bytes = _lib.call("ps_spectral_workspace_bytes", self.host.data_ptr())
        if self.ws_bytes == 0:
            raise RuntimeError("ps_spectral_workspace_bytes: not a table")

    def views(self, flat, like):
        """Layer k's region of a flat buffer in the shape and the strides of like[k]"""
        return tuple(torch.as_strided(flat, w.shape, w.stride(), self.elem[k]) for k, w in enumerate(like))


def _table(layers, device):
    key = (device,) + tuple((w.data_ptr(), u.data_ptr(), v.data_ptr(), tuple(w.shape), it, eps, inter) for w, u, v, it, eps, inter in layers)
    table = _TABLES.get(key)
    if table is None:
        if len(_TABLES) >= _MAX_TABLES:
            _TABLES.clear()
        table = _TABLES[key] = _Table(layers, device)
    return table


class _Normalise(torch.autograd.Function):
    """table, all weight_orig -> all weight_orig / sigma (views of one buffer).  Keeps that buffer, sigma and copies of the u and v sigma
    was computed with: a later forward's update of weight_u / weight_v in place must not reach this one's backward."""

    @staticmethod
    def forward(ctx, table, *weights):
        dev = weights[0].device
        new = lambda n: torch.empty(int(n), dtype=torch.float32, device=dev)
        w_sn, u_saved, v_saved, sigma = new(table.elem[-1]), new(table.row[-1]), new(table.col[-1]), new(table.n)
        ws = _WS.get(dev, table.ws_bytes)
        _lib.call("ps_spectral_forward_f32", table.host.data_ptr(), table.device, w_sn, u_saved, v_saved, sigma, ws, ws.numel())
        ctx.table, ctx.kept = table, (w_sn, u_saved, v_saved, sigma)
        ctx.like = [(w.shape, w.stride()) for w in weights]
        ctx.set_materialize_grads(False)
        return table.views(w_sn, weights)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        table = ctx.table
        w_sn, u_saved, v_saved, sigma = ctx.kept
        # a gradient in the layout of its weight (what a convolution's backward returns for a channels-last weight is that already)
        grads = [None if g is None else (g if g.dtype == torch.float32 and g.stride() == stride
                                         else torch.empty_strided(shape, stride, dtype=torch.float32, device=g.device).copy_(g))
                 for g, (shape, stride) in zip(grads, ctx.like)]
        ptrs = (ctypes.c_void_p * table.n)(*[None if g is None else g.data_ptr() for g in grads])
        dw = torch.empty_like(w_sn)
        ws = _WS.get(w_sn.device, table.ws_bytes)
        _lib.call("ps_spectral_backward_f32", table.host.data_ptr(), table.device, ptrs, w_sn, u_saved, v_saved, sigma, dw, ws, ws.numel())
        return (None,) + tuple(torch.as_strided(dw, shape, stride, table.elem[k]) for k, (shape, stride) in enumerate(ctx.like))


def normalise(modules, opt=None):
    """One batched pass over those of `modules` that _layer() takes (at most MAX_LAYERS per call of the library): their power iteration
    where they iterate, their normalised weight left pending on each.  Differentiable once in every weight_orig; without grad mode forward
    only.  -> the modules taken.  The caller decides WHETHER (active()); this function does not look at the switch."""
    modules = list({id(m): m for m in modules}.values())       # (a module listed twice iterates once)
    taken = [(m, layer) for m, layer in ((m, _layer(m)) for m in modules) if layer is not None]
    for dev in {layer[0].device for _, layer in taken}:
        group = [(m, layer) for m, layer in taken if layer[0].device == dev]
        with torch.cuda.device(dev):
            for i in range(0, len(group), MAX_LAYERS):
                chunk = group[i:i + MAX_LAYERS]
                layers = [layer for _, layer in chunk]
                outs = _Normalise.apply(_table(layers, dev), *[layer[0] for layer in layers])
                # the hook's copy_ / out= move the version counters of u and v: what is cached from them (routing.cached) must see it
                torch.autograd.graph.increment_version([t for _, u, v, it, _, _ in layers if it for t in (u, v)])
                for (m, _), w in zip(chunk, outs):
                    leave_pending(m, w)
    return [m for m, _ in taken]


def sn_modules(net):
    """The modules of `net` that may be under spectral norm: every Conv2d, Linear and _SNConv (normalise() sorts out which are)"""
    from .discriminators import _SNConv
    return [m for m in net.modules() if type(m) in (nn.Conv2d, nn.Linear, _SNConv)]
