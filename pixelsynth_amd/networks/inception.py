"""The FID network: Inception-v3 as pytorch_fid runs it at its default dims = 2048 -- torchvision's Inception3 trunk without AuxLogits
and fc, with pytorch_fid's four changed blocks (the average pools of Mixed_5b .. 6e and Mixed_7b count only the taps inside the map,
Mixed_7c's pool branch is a max-pool) --, in eval mode, ending in the mean over the 8 x 8 map: 2048 features per image.

FIDInception(weights=PATH or state dict) holds torchvision's keys (<block>.<branch>.conv.weight, <block>.<branch>.bn.{weight, bias,
running_mean, running_var}) and loads a pt_inception-2015-12-05-*.pth-style state dict; fc.*, AuxLogits.* and num_batches_tracked are
ignored, a missing or misshapen trunk key is an error that names it.  Nothing is downloaded: without weights the parameters keep torch's
initialisation.  torch_forward(x) is the plain torch formula (the fallback and the yardstick of the HIP path, fid.py);
hip_layers(device) the 94 convolutions with their BatchNorm folded, packed for csrc/fid.hip, once per set of weights.

Every "conv" is Conv2d(bias=False) + BatchNorm2d(eps=0.001) + ReLU.  NETWORK lists the blocks: a block is a list of branches whose
outputs are concatenated in order; a branch is a list of steps, each the name of a convolution, a pool ("max2": 3 x 3 stride 2,
"max1": 3 x 3 stride 1 padding 1, "avg": 3 x 3 stride 1 padding 1 over the taps inside the map) or a pair of names (both applied to
the same input, concatenated)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .routing import cached

SIZE, DIMS, BN_EPS = 299, 2048, 0.001


def _a(cin, pool):
    return {"branch1x1": (cin, 64, 1), "branch5x5_1": (cin, 48, 1), "branch5x5_2": (48, 64, 5, 1, 2),
            "branch3x3dbl_1": (cin, 64, 1), "branch3x3dbl_2": (64, 96, 3, 1, 1), "branch3x3dbl_3": (96, 96, 3, 1, 1),
            "branch_pool": (cin, pool, 1)}


def _c(c7):
    return {"branch1x1": (768, 192, 1), "branch7x7_1": (768, c7, 1), "branch7x7_2": (c7, c7, (1, 7), 1, (0, 3)),
            "branch7x7_3": (c7, 192, (7, 1), 1, (3, 0)), "branch7x7dbl_1": (768, c7, 1), "branch7x7dbl_2": (c7, c7, (7, 1), 1, (3, 0)),
            "branch7x7dbl_3": (c7, c7, (1, 7), 1, (0, 3)), "branch7x7dbl_4": (c7, c7, (7, 1), 1, (3, 0)),
            "branch7x7dbl_5": (c7, 192, (1, 7), 1, (0, 3)), "branch_pool": (768, 192, 1)}


def _e(cin):
    return {"branch1x1": (cin, 320, 1), "branch3x3_1": (cin, 384, 1), "branch3x3_2a": (384, 384, (1, 3), 1, (0, 1)),
            "branch3x3_2b": (384, 384, (3, 1), 1, (1, 0)), "branch3x3dbl_1": (cin, 448, 1), "branch3x3dbl_2": (448, 384, 3, 1, 1),
            "branch3x3dbl_3a": (384, 384, (1, 3), 1, (0, 1)), "branch3x3dbl_3b": (384, 384, (3, 1), 1, (1, 0)),
            "branch_pool": (cin, 192, 1)}


# module -> {branch: (Ci, Co, kernel, stride = 1, padding = 0)}; a stem convolution is a module of its own (branch None)
MODULES = {
    "Conv2d_1a_3x3": {None: (3, 32, 3, 2)}, "Conv2d_2a_3x3": {None: (32, 32, 3)}, "Conv2d_2b_3x3": {None: (32, 64, 3, 1, 1)},
    "Conv2d_3b_1x1": {None: (64, 80, 1)}, "Conv2d_4a_3x3": {None: (80, 192, 3)},
    "Mixed_5b": _a(192, 32), "Mixed_5c": _a(256, 64), "Mixed_5d": _a(288, 64),
    "Mixed_6a": {"branch3x3": (288, 384, 3, 2), "branch3x3dbl_1": (288, 64, 1), "branch3x3dbl_2": (64, 96, 3, 1, 1),
                 "branch3x3dbl_3": (96, 96, 3, 2)},
    "Mixed_6b": _c(128), "Mixed_6c": _c(160), "Mixed_6d": _c(160), "Mixed_6e": _c(192),
    "Mixed_7a": {"branch3x3_1": (768, 192, 1), "branch3x3_2": (192, 320, 3, 2), "branch7x7x3_1": (768, 192, 1),
                 "branch7x7x3_2": (192, 192, (1, 7), 1, (0, 3)), "branch7x7x3_3": (192, 192, (7, 1), 1, (3, 0)),
                 "branch7x7x3_4": (192, 192, 3, 2)},
    "Mixed_7b": _e(1280), "Mixed_7c": _e(2048),
}


def _blocks():
    m = lambda mod, *names: [f"{mod}.{n}" for n in names]
    out = [("stem", [["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "max2", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "max2"]])]
    for mod in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        out.append((mod, [m(mod, "branch1x1"), m(mod, "branch5x5_1", "branch5x5_2"),
                          m(mod, "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), ["avg"] + m(mod, "branch_pool")]))
    out.append(("Mixed_6a", [m("Mixed_6a", "branch3x3"), m("Mixed_6a", "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), ["max2"]]))
    for mod in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        out.append((mod, [m(mod, "branch1x1"), m(mod, "branch7x7_1", "branch7x7_2", "branch7x7_3"),
                          m(mod, *["branch7x7dbl_%d" % i for i in range(1, 6)]), ["avg"] + m(mod, "branch_pool")]))
    out.append(("Mixed_7a", [m("Mixed_7a", "branch3x3_1", "branch3x3_2"),
                             m("Mixed_7a", *["branch7x7x3_%d" % i for i in range(1, 5)]), ["max2"]]))
    for mod, pool in (("Mixed_7b", "avg"), ("Mixed_7c", "max1")):
        out.append((mod, [m(mod, "branch1x1"), m(mod, "branch3x3_1") + [tuple(m(mod, "branch3x3_2a", "branch3x3_2b"))],
                          m(mod, "branch3x3dbl_1", "branch3x3dbl_2") + [tuple(m(mod, "branch3x3dbl_3a", "branch3x3dbl_3b"))],
                          [pool] + m(mod, "branch_pool")]))
    return out


NETWORK = _blocks()
POOLS = ("max2", "max1", "avg")


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def conv_specs():
    """-> {name: (Ci, Co, (KH, KW), stride, (ph, pw))} of the 94 convolutions, in the modules' order; name = "<block>.<branch>" (the
    prefix of its state-dict keys) or the stem convolution's own name."""
    out = {}
    for mod, branches in MODULES.items():
        for br, spec in branches.items():
            ci, co, k, s, p = tuple(spec) + (1, 0)[len(spec) - 3:]
            out[mod if br is None else f"{mod}.{br}"] = (ci, co, _pair(k), s, _pair(p))
    return out


class BasicConv2d(nn.Module):
    def __init__(self, ci, co, kernel, stride, padding):
        super().__init__()
        self.conv = nn.Conv2d(ci, co, kernel, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(co, eps=BN_EPS)

    def forward(self, x):        # eval mode whatever the module's flag says: the running statistics
        bn = self.bn
        return F.relu(F.batch_norm(self.conv(x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))


def _pool(x, kind):
    if kind == "max2":
        return F.max_pool2d(x, 3, 2)
    if kind == "max1":
        return F.max_pool2d(x, 3, 1, 1)
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


class FIDInception(nn.Module):
    def __init__(self, weights=None, use_gpu=False):
        super().__init__()
        specs = conv_specs()
        for mod, branches in MODULES.items():
            if None in branches:
                self.add_module(mod, BasicConv2d(*specs[mod]))
            else:
                box = nn.Module()
                for br in branches:
                    box.add_module(br, BasicConv2d(*specs[f"{mod}.{br}"]))
                self.add_module(mod, box)
        if weights is not None:
            self.load_weights(weights)
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        if use_gpu:
            self.cuda()

    def conv(self, name):
        """The BasicConv2d called `name` in conv_specs()."""
        m = self
        for part in name.split("."):
            m = getattr(m, part)
        return m

    def load_weights(self, weights):
        """weights: a path (torch.load on the CPU, tensors only) or a state dict with torchvision's Inception3 keys."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        skip = lambda k: k.startswith(("fc.", "AuxLogits.")) or k.endswith("num_batches_tracked")
        given = {k: v for k, v in weights.items() if not skip(k)}
        own = {k: v for k, v in self.state_dict().items() if not skip(k)}
        for k, v in own.items():
            if k not in given:
                raise KeyError(f"FIDInception: the state dict has no {k}")
            if tuple(given[k].shape) != tuple(v.shape):
                raise ValueError(f"FIDInception: {k} has shape {tuple(given[k].shape)}, expected {tuple(v.shape)}")
        extra = sorted(set(given) - set(own))
        if extra:
            raise KeyError(f"FIDInception: unexpected key {extra[0]} in the state dict")
        self.load_state_dict({k: torch.as_tensor(v) for k, v in given.items()}, strict=False)

    # ---- the torch formula
    def torch_forward(self, x):
        """x (N, 3, H, W) float images in [0, 1] on any device -> (N, 2048) features."""
        if tuple(x.shape[2:]) != (SIZE, SIZE):
            x = F.interpolate(x, size=(SIZE, SIZE), mode="bilinear", align_corners=False)
        x = 2 * x - 1
        for _, branches in NETWORK:
            outs = []
            for steps in branches:
                h = x
                for step in steps:
                    if isinstance(step, tuple):
                        h = torch.cat([self.conv(n)(h) for n in step], 1)
                    else:
                        h = _pool(h, step) if step in POOLS else self.conv(step)(h)
                outs.append(h)
            x = outs[0] if len(outs) == 1 else torch.cat(outs, 1)
        return x.mean((2, 3))

    def forward(self, x):
        """x (N, 3, H, W) float32 in [0, 1] or uint8 -> (N, 2048): the HIP path on the ROCm device (fid.inception_features), the torch
        formula on the CPU."""
        if x.is_cuda:
            from ..fid import inception_features
            return inception_features(self, x)
        return self.torch_forward(x.float() / 255.0 if x.dtype == torch.uint8 else x)

    # ---- the HIP path (fid.py)
    def folded(self, name):
        """-> (w' (Co, Ci, KH, KW), b' (Co)) fp32 of convolution `name` with its BatchNorm folded in, computed in fp64 and rounded once:
        w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps)."""
        m = self.conv(name)
        g = m.bn.weight.detach().double() / torch.sqrt(m.bn.running_var.detach().double() + m.bn.eps)
        w = m.conv.weight.detach().double() * g.view(-1, 1, 1, 1)
        b = m.bn.bias.detach().double() - m.bn.running_mean.detach().double() * g
        return w.float(), b.float()

    def hip_layers(self, device):
        """{name: the folded convolution packed by fid.pack_conv} on `device`, once per set of weights and device (routing.cached); None
        when a convolution is outside what ps_fid_conv takes (torch then runs)."""
        from .. import fid
        tensors = [t for n in conv_specs() for m in (self.conv(n),)
                   for t in (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)]

        def pack():
            layers = {}
            for name, (ci, co, k, s, p) in conv_specs().items():
                w, b = self.folded(name)
                layers[name] = fid.pack_conv(w.to(device), b.to(device), s, p)
                if layers[name] is None:
                    return None
            return layers
        return cached(self, f"_hip_cache_{device}", tensors, pack)


def conv_shapes():
    """-> [(name, KH, KW, stride, ph, pw, Ci, Co, H, W)] of the 94 convolutions at the network's 299 x 299 input, H x W the map a
    convolution reads, in running order (what tools/fid_time.py tabulates)."""
    specs, out = conv_specs(), []

    def walk(step, H, W, C):
        if isinstance(step, tuple):
            shapes = [walk(s, H, W, C) for s in step]
            return shapes[0][:2] + (sum(s[2] for s in shapes),)
        if step in POOLS:
            return ((H - 3) // 2 + 1, (W - 3) // 2 + 1, C) if step == "max2" else (H, W, C)
        ci, co, (kh, kw), s, (ph, pw) = specs[step]
        out.append((step, kh, kw, s, ph, pw, ci, co, H, W))
        return ((H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1, co)

    shape = (SIZE, SIZE, 3)
    for _, branches in NETWORK:
        ends = []
        for steps in branches:
            s = shape
            for step in steps:
                s = walk(step, *s)
            ends.append(s)
        shape = ends[0][:2] + (sum(e[2] for e in ends),)
    return out
