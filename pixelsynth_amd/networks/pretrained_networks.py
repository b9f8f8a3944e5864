"""PercSim's network, with the interface of the reference's models/networks/pretrained_networks.py (PNet, vgg16, normalize_tensor,
cos_sim: the same names, arguments, state-dict keys and return values).  Only the VGG16 network is provided.

The score of a pair is the sum over five taps of VGG16 (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) of 1 - the mean over pixels of
the cosine between the two images' feature vectors, each vector divided by (its norm + 1e-10); inputs are in [-1, 1] and are
standardised per channel by shift (-0.030, -0.088, -0.188) and scale (0.458, 0.448, 0.450) first.

Weights are never downloaded.  PNet(weights=...) takes a path or a state dict, in torchvision's VGG16 format (features.{0, 2, 5, ...,
28}.weight / .bias; classifier.* ignored) or PNet's own (net.slice1.0.weight, ...).  Without weights and with pnet_rand=False, the file
torchvision itself would have cached is used: torch.hub.get_dir()/checkpoints/vgg16-397923af.pth (FileNotFoundError if it is not
there).  pnet_rand=True gives torchvision's initialisation.

forward(in0, in1) runs on the HIP kernels (the split-fp16 convolutions of csrc/conv_f16x3.hip and csrc/conv_thin.hip, the taps of
csrc/percsim.hip; perceptual.py) when both inputs are CUDA fp32 (N, 3, H, W) with H and W multiples of 256, no input requires grad,
the weights are on the inputs' device and fp16 can hold them, and networks.f16x3.decoder_conv("fp32") is not in effect; that pass is a
guarded scope (f16x3.checked: an activation beyond fp16's range warns and reruns through torch).  Everything else runs the torch
formula (torch_forward), on any device.
"""
import os
from collections import namedtuple

import torch
import torch.nn as nn

VGG16_FILE = "vgg16-397923af.pth"    # torchvision's name of its VGG16 checkpoint
# torchvision's vgg16().features (configuration "D"): 3 x 3 convolutions (each followed by a ReLU) and "M" 2 x 2 max-pools, 31 modules
_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)    # the indices of the 13 convolutions in features
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))     # slice1 .. slice5 = features[lo:hi], the last one ends at relu5_3
TAPS = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
_Taps = namedtuple("VggOutputs", TAPS)
_SHIFT = (-0.030, -0.088, -0.188)
_SCALE = (0.458, 0.448, 0.450)


def normalize_tensor(in_feat, eps=1e-10):
    """(N, C, H, W) -> each pixel's channel vector divided by (its Euclidean norm + eps)."""
    n = in_feat.pow(2).sum(1, keepdim=True).sqrt()
    return in_feat / (n + eps)


def cos_sim(in0, in1):
    """(N, C, H, W) x 2 -> (N,): the channel-wise cosine of the normalised maps, averaged over rows, then over columns."""
    per_pixel = (normalize_tensor(in0) * normalize_tensor(in1)).sum(1)      # (N, H, W)
    return per_pixel.mean(1).mean(1)


def vgg16_features():
    """torchvision's vgg16().features as a list of modules, with torchvision's initialisation (Kaiming normal, fan_out, zero bias)."""
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
    return layers


class vgg16(nn.Module):
    """VGG16's features up to relu5_3 as five nn.Sequential slices named by their torchvision indices (slice1.0, slice1.2, slice2.5,
    ...).  forward -> a namedtuple of the five tapped maps.  `pretrained` is accepted for the reference's signature; PNet loads the
    weights (module docstring)."""

    def __init__(self, requires_grad=False, pretrained=True):
        super().__init__()
        feats = vgg16_features()
        self.N_slices = len(SLICES)
        for s, (lo, hi) in enumerate(SLICES):
            self.add_module(f"slice{s + 1}", nn.Sequential())
            for i in range(lo, hi):
                getattr(self, f"slice{s + 1}").add_module(str(i), feats[i])
        for p in self.parameters():
            p.requires_grad_(requires_grad)

    def slices(self):
        return [getattr(self, f"slice{s + 1}") for s in range(self.N_slices)]

    def forward(self, X):
        taps = []
        for sl in self.slices():
            X = sl(X)
            taps.append(X)
        return _Taps(*taps)

    def convs(self):
        """The 13 Conv2d modules in order."""
        return [m for sl in self.slices() for m in sl if isinstance(m, nn.Conv2d)]


def default_weights_path():
    """Where torchvision caches its VGG16 checkpoint: torch.hub.get_dir()/checkpoints/vgg16-397923af.pth (TORCH_HOME decides)."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", VGG16_FILE)


def vgg16_slices_state_dict(sd):
    """A torchvision VGG16 state dict (features.*; classifier.* ignored) or a PNet / vgg16 one -> vgg16's keys (slice1.0.weight, ...)."""
    if not any(k.startswith("features.") for k in sd):
        return {k[4:] if k.startswith("net.") else k: v for k, v in sd.items()}
    slice_of = {i: s + 1 for s, (lo, hi) in enumerate(SLICES) for i in range(lo, hi)}
    out = {}
    for k, v in sd.items():
        if k.startswith("features."):
            _, i, what = k.split(".")
            if int(i) not in CONVS:
                raise KeyError(f"unexpected key {k} in a VGG16 state dict")
            out[f"slice{slice_of[int(i)]}.{i}.{what}"] = v
    return out


class PNet(nn.Module):
    """PercSim's network, every channel weighted alike.  pnet_type "vgg" / "vgg16" only; weights: a path or a state dict (module
    docstring).  shift / scale are plain attributes (not in the state dict); use_gpu moves everything to the current CUDA device."""

    def __init__(self, pnet_type="vgg", pnet_rand=False, use_gpu=True, weights=None):
        super().__init__()
        self.use_gpu, self.pnet_type, self.pnet_rand = use_gpu, pnet_type, pnet_rand
        self.shift = torch.tensor(_SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
        self.scale = torch.tensor(_SCALE, dtype=torch.float32).view(1, 3, 1, 1)
        if pnet_type in ("alex", "squeeze") or pnet_type[:-2] == "resnet":
            raise NotImplementedError(f"PNet: only the VGG16 network is provided, not {pnet_type!r}")
        if pnet_type not in ("vgg", "vgg16"):
            raise ValueError(f"PNet: unknown pnet_type {pnet_type!r}")
        self.net = vgg16(requires_grad=False, pretrained=not pnet_rand)
        if weights is None and not pnet_rand:
            weights = default_weights_path()
            if not os.path.exists(weights):
                raise FileNotFoundError(f"PNet: no VGG16 weights at {weights} (torchvision's cache under TORCH_HOME); pass weights= a "
                                        f"{VGG16_FILE} file or a state dict (nothing is downloaded)")
        if weights is not None:
            self.load_weights(weights)
        self.L = self.net.N_slices
        self._hip_cache = None
        if use_gpu:
            self.cuda()

    def load_weights(self, weights):
        """weights: a path (torch.load on the CPU, tensors only) or a state dict, in torchvision's or PNet's format."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        self.net.load_state_dict(vgg16_slices_state_dict(weights))
        self._hip_cache = None

    def _apply(self, fn, *args, **kwargs):      # .cuda() / .to() / .float(): shift and scale follow the network
        out = super()._apply(fn, *args, **kwargs)
        self.shift, self.scale = fn(self.shift), fn(self.scale)
        return out

    # ---- the HIP path (perceptual.py)
    def hip_takes(self, in0, in1):
        from . import f16x3
        if f16x3.forced_mode() == "fp32":
            return False
        for t in (in0, in1):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.size(0) >= 1 and t.size(1) == 3
                    and t.size(2) % 256 == 0 and t.size(3) % 256 == 0 and not t.requires_grad):
                return False
        dev = self.net.convs()[0].weight.device
        return in0.shape == in1.shape and in0.device == in1.device == dev and self.hip_layers(dev) is not None

    def hip_layers(self, device):
        """The 13 convolutions prepared for the kernels -- conv1_1 as a [ky][kx][ci of 4][co] fp32 weight and its bias, the others
        packed by f16x3.pack3x3 with their bias --, once per set of weights; None when fp16 cannot hold a weight (torch then runs)."""
        from . import f16x3
        convs = self.net.convs()
        key = (str(device),) + tuple((c.weight.data_ptr(), c.weight._version, c.bias.data_ptr(), c.bias._version) for c in convs)
        if self._hip_cache is None or self._hip_cache[0] != key:
            with torch.no_grad():
                w0 = convs[0].weight.detach().float()
                w0 = torch.cat([w0, w0.new_zeros(w0.size(0), 1, 3, 3)], 1).permute(2, 3, 1, 0).contiguous()
                top = float(w0.abs().max())
                try:
                    if not top < 6.0e4:
                        raise ValueError("split-fp16 convolution: a weight fp16 cannot hold")
                    packed = [f16x3.pack3x3(c.weight.detach().float(), c.bias.detach().float()) for c in convs[1:]]
                    layers = dict(w0=w0, b0=convs[0].bias.detach().float().contiguous(), packed=packed)
                except ValueError:
                    layers = None
            self._hip_cache = (key, layers, [c.weight for c in convs] + [c.bias for c in convs])   # (keeps the keyed tensors alive)
        return self._hip_cache[1]

    # ---- the torch formula
    def torch_forward(self, in0, in1, retPerLayer=False):
        """The score through torch modules on any device: standardise, run both images through the slices, 1 - cos_sim per tap."""
        shift, scale = self.shift.to(in0.device), self.scale.to(in0.device)
        f0 = self.net((in0 - shift) / scale)
        f1 = self.net((in1 - shift) / scale)
        per_layer = [1.0 - cos_sim(a, b) for a, b in zip(f0, f1)]
        total = per_layer[0]
        for s in per_layer[1:]:
            total = total + s
        return (total, per_layer) if retPerLayer else total

    def forward(self, in0, in1, retPerLayer=False):
        """in0, in1 (N, 3, H, W) in [-1, 1] -> (N,) the sum over the five taps of 1 - cos_sim; retPerLayer: (that, [5 x (N,)])."""
        if self.hip_takes(in0, in1):
            from ..perceptual import pnet_pairs
            total, layers = pnet_pairs(self, in0, in1)
            return (total, list(layers.unbind(1))) if retPerLayer else total
        return self.torch_forward(in0, in1, retPerLayer)
