"""The content loss's network, with the interface of the reference's VGG19 (models/networks/architectures.py:52-85): torchvision's
vgg19().features[0:30] as five nn.Sequential slices whose modules carry their torchvision indices (slice1.0, slice2.2, slice2.5, ...,
slice5.28); forward(X) -> [relu1_1, relu2_1, relu3_1, relu4_1, relu5_1].  The input is used as it comes: the reference normalises
nothing.

Weights follow PNet's conventions (pretrained_networks.py), not torchvision's: nothing is downloaded.  VGG19(weights=...) takes a path or
a state dict, in torchvision's VGG19 format (features.{0, 2, 5, ..., 28}.weight / .bias; features.30 and later and classifier.* ignored)
or the class's own keys (slice1.0.weight, ...).  Without weights and with rand=False, the file torchvision itself would have cached is
used: torch.hub.get_dir()/checkpoints/vgg19-dcbb9e9d.pth (FileNotFoundError if it is not there).  rand=True gives torchvision's
initialisation.

hip_layers(device) prepares the thirteen convolutions for the kernels of the content loss (losses/synthesis.py), forward and backward.
"""
import os

import torch
import torch.nn as nn

VGG19_FILE = "vgg19-dcbb9e9d.pth"    # torchvision's name of its VGG19 checkpoint
# torchvision's vgg19().features (configuration "E") up to relu5_1: 30 modules
_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512)
CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)    # the indices of the 13 convolutions in features
POOLS = (4, 9, 18, 27)
SLICES = ((0, 2), (2, 7), (7, 12), (12, 21), (21, 30))      # slice1 .. slice5 = features[lo:hi], each ends at its relu*_1
TAPS = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1")
TAPPED = (0, 2, 4, 8, 12)            # which of the 13 convolutions (counted 0 .. 12) feed a tap
POOL_BEFORE = (2, 4, 8, 12)          # which of them read a max-pooled map


def vgg19_features():
    """torchvision's vgg19().features[0:30] as a list of modules, with torchvision's initialisation (Kaiming normal, fan_out, zero bias)."""
    layers, c = [], 3
    for v in _CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(c, v, kernel_size=3, padding=1)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.zeros_(conv.bias)
        layers += [conv, nn.ReLU(inplace=True)]
        c = v
    assert len(layers) == SLICES[-1][1]
    return layers


def default_weights_path():
    """Where torchvision caches its VGG19 checkpoint: torch.hub.get_dir()/checkpoints/vgg19-dcbb9e9d.pth (TORCH_HOME decides)."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", VGG19_FILE)


def vgg19_slices_state_dict(sd):
    """A torchvision VGG19 state dict (features.*; features.30 and later and classifier.* ignored) or a VGG19 one -> VGG19's keys"""
    if not any(k.startswith("features.") for k in sd):
        return dict(sd)
    slice_of = {i: s + 1 for s, (lo, hi) in enumerate(SLICES) for i in range(lo, hi)}
    out = {}
    for k, v in sd.items():
        if k.startswith("features."):
            _, i, what = k.split(".")
            if int(i) >= SLICES[-1][1]:
                continue
            if int(i) not in CONVS:
                raise KeyError(f"unexpected key {k} in a VGG19 state dict")
            out[f"slice{slice_of[int(i)]}.{i}.{what}"] = v
    return out


class VGG19(nn.Module):
    """VGG19's features up to relu5_1 (module docstring).  requires_grad=False freezes the parameters, as the reference does for its loss."""

    def __init__(self, requires_grad=False, weights=None, rand=False):
        super().__init__()
        feats = vgg19_features()
        for s, (lo, hi) in enumerate(SLICES):
            self.add_module(f"slice{s + 1}", nn.Sequential())
            for i in range(lo, hi):
                getattr(self, f"slice{s + 1}").add_module(str(i), feats[i])
        self._hip_cache = None
        if weights is None and not rand:
            weights = default_weights_path()
            if not os.path.exists(weights):
                raise FileNotFoundError(f"VGG19: no VGG19 weights at {weights} (torchvision's cache under TORCH_HOME); pass weights= a "
                                        f"{VGG19_FILE} file or a state dict (nothing is downloaded)")
        if weights is not None:
            self.load_weights(weights)
        if not requires_grad:
            for p in self.parameters():
                p.requires_grad_(False)

    def load_weights(self, weights):
        """weights: a path (torch.load on the CPU, tensors only) or a state dict, in torchvision's or VGG19's format."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        self.load_state_dict(vgg19_slices_state_dict(weights))
        self._hip_cache = None

    def slices(self):
        return [getattr(self, f"slice{s + 1}") for s in range(len(SLICES))]

    def convs(self):
        """The 13 Conv2d modules in order."""
        return [m for sl in self.slices() for m in sl if isinstance(m, nn.Conv2d)]

    def forward(self, X):
        out = []
        for sl in self.slices():
            X = sl(X)
            out.append(X)
        return out

    def hip_layers(self, device):
        """The 13 convolutions prepared for the kernels, once per set of weights (keyed as PNet.hip_layers keys them): w0, conv1_1 as a
        [ky][kx][ci of 4][co] fp32 weight, and b0 its bias; packed, the other twelve by f16x3.pack3x3 with their bias; flipped, the
        twelve packs of W'[c, t, o] = W[o, 8 - t, c] the grad_input convolutions run on; w0_flipped, conv1_1's flipped 64 -> 3 weight
        [ky][kx][co][ci of 3], as ps_conv3x3_thin_out_nhwc_f32 reads it.  None when fp16 cannot hold a weight (torch then runs)."""
        from . import f16x3
        convs = self.convs()
        key = (str(device),) + tuple((c.weight.data_ptr(), c.weight._version, c.bias.data_ptr(), c.bias._version) for c in convs)
        if self._hip_cache is None or self._hip_cache[0] != key:
            with torch.no_grad():
                w = convs[0].weight.detach().float()
                w0 = torch.cat([w, w.new_zeros(w.size(0), 1, 3, 3)], 1).permute(2, 3, 1, 0).contiguous()
                top = float(w0.abs().max())
                try:
                    if not top < 6.0e4:
                        raise ValueError("split-fp16 convolution: a weight fp16 cannot hold")
                    packed = [f16x3.pack3x3(c.weight.detach().float(), c.bias.detach().float()) for c in convs[1:]]
                    flipped = [f16x3.pack3x3(c.weight.detach().float().flip(2, 3).transpose(0, 1), check=False) for c in convs[1:]]
                    layers = dict(w0=w0, b0=convs[0].bias.detach().float().contiguous(), packed=packed, flipped=flipped,
                                  w0_flipped=w.flip(2, 3).permute(2, 3, 0, 1).contiguous())
                except ValueError:
                    layers = None
            self._hip_cache = (key, layers, [c.weight for c in convs] + [c.bias for c in convs])   # (keeps the keyed tensors alive)
        return self._hip_cache[1]
