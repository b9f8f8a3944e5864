"""The VGG trunk behind PercSim's vgg16 (pretrained_networks.py) and the content loss's VGG19 (vgg19.py): torchvision's features built
from a configuration, cut into five nn.Sequential slices whose modules carry their torchvision indices; the translation of a
torchvision state dict into the slices' keys; where weights come from (a path, a state dict, or the file torchvision itself would have
cached: nothing is downloaded); and the thirteen convolutions as the split-fp16 kernels read them (prepare_convs).  Each network is a
thin declaration over this: its tables (_CFG, CONVS, SLICES, TAPS), its file name and its return type.
"""
import os

import torch
import torch.nn as nn


def features(cfg, upto):
    """torchvision's vgg*().features[0:upto] for configuration `cfg` (channel counts of 3 x 3 convolutions, each followed by a ReLU, and
    "M" 2 x 2 max-pools) as a list of modules, with torchvision's initialisation (Kaiming normal, fan_out, zero bias)."""
    layers, c = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(c, v, kernel_size=3, padding=1)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.zeros_(conv.bias)
        layers += [conv, nn.ReLU(inplace=True)]
        c = v
    assert len(layers) >= upto
    return layers[:upto]


class Slices(nn.Module):
    """features(cfg, .) as nn.Sequential slices slice1 .. sliceN = features[lo:hi] for (lo, hi) of `slices`, each module named by its
    torchvision index (slice1.0, slice1.2, slice2.5, ...).  forward -> the list of the slices' outputs."""

    def __init__(self, cfg, slices, requires_grad=False):
        super().__init__()
        feats = features(cfg, slices[-1][1])
        self.N_slices = len(slices)
        for s, (lo, hi) in enumerate(slices):
            self.add_module(f"slice{s + 1}", nn.Sequential())
            for i in range(lo, hi):
                getattr(self, f"slice{s + 1}").add_module(str(i), feats[i])
        for p in self.parameters():
            p.requires_grad_(requires_grad)

    def slices(self):
        return [getattr(self, f"slice{s + 1}") for s in range(self.N_slices)]

    def convs(self):
        """The Conv2d modules in order."""
        return [m for sl in self.slices() for m in sl if isinstance(m, nn.Conv2d)]

    def forward(self, X):
        out = []
        for sl in self.slices():
            X = sl(X)
            out.append(X)
        return out


def slices_state_dict(sd, name, convs, slices, own_prefix="", ignore_after=False):
    """A torchvision state dict (features.*; classifier.* ignored) -> the keys of a Slices(., slices) whose convolutions sit at the
    indices `convs` (slice1.0.weight, ...); a dict without features.* keys is the network's own and only loses `own_prefix`.  KeyError,
    in `name`'s name, for a features.N that is no convolution -- with ignore_after, only below the last slice's end: later ones are
    ignored."""
    if not any(k.startswith("features.") for k in sd):
        return {k[len(own_prefix):] if own_prefix and k.startswith(own_prefix) else k: v for k, v in sd.items()}
    slice_of = {i: s + 1 for s, (lo, hi) in enumerate(slices) for i in range(lo, hi)}
    out = {}
    for k, v in sd.items():
        if k.startswith("features."):
            _, i, what = k.split(".")
            if ignore_after and int(i) >= slices[-1][1]:
                continue
            if int(i) not in convs:
                raise KeyError(f"unexpected key {k} in a {name} state dict")
            out[f"slice{slice_of[int(i)]}.{i}.{what}"] = v
    return out


def load(weights):
    """weights: a path (torch.load on the CPU, tensors only) or a state dict -> the state dict"""
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    return weights


def default_weights_path(file_name):
    """Where torchvision caches the checkpoint it calls `file_name`: torch.hub.get_dir()/checkpoints/file_name (TORCH_HOME decides)."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", file_name)


def cached_weights(owner, name, file_name):
    """default_weights_path(file_name) for `owner`'s network `name`; FileNotFoundError if it is not there (nothing is downloaded)"""
    path = default_weights_path(file_name)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{owner}: no {name} weights at {path} (torchvision's cache under TORCH_HOME); pass weights= a "
                                f"{file_name} file or a state dict (nothing is downloaded)")
    return path


def prepare_convs(convs, device, backward=False):
    """The convolutions of a trunk prepared for the kernels on `device`: w0, the first one (3 -> 64) as a [ky][kx][ci of 4][co] fp32 weight,
    and b0 its bias; packed, the others by f16x3.pack3x3 with their bias.  backward: also flipped, their packs of W'[c, t, o] = W[o, 8 - t,
    c] that the grad_input convolutions run on, and w0_flipped, the first one's flipped 64 -> 3 weight [ky][kx][co][ci of 3], as
    ps_conv3x3_thin_out_nhwc_f32 reads it.  None when fp16 cannot hold a weight (torch then runs)."""
    from . import f16x3
    with torch.no_grad():
        weights = [c.weight.detach().float().to(device) for c in convs]
        biases = [c.bias.detach().float().to(device) for c in convs]
        w0 = torch.cat([weights[0], weights[0].new_zeros(weights[0].size(0), 1, 3, 3)], 1).permute(2, 3, 1, 0).contiguous()
        try:
            f16x3.check_weight(w0)
            layers = dict(w0=w0, b0=biases[0].contiguous(), packed=[f16x3.pack3x3(w, b) for w, b in zip(weights[1:], biases[1:])])
            if backward:
                layers.update(flipped=[f16x3.pack3x3(w.flip(2, 3).transpose(0, 1), check=False) for w in weights[1:]],
                              w0_flipped=weights[0].flip(2, 3).permute(2, 3, 0, 1).contiguous())
        except ValueError:
            return None
    return layers
