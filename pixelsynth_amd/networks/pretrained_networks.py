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

The trunk -- the features builder, the slices, the key translation, the loading and the preparation of the convolutions -- is
networks/vgg.py's, shared with the content loss's VGG19 (vgg19.py); here are VGG16's tables and PNet.
"""
from collections import namedtuple

import torch
import torch.nn as nn

from . import vgg
from .routing import cached

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


class vgg16(vgg.Slices):
    """VGG16's features up to relu5_3 as five nn.Sequential slices named by their torchvision indices (vgg.Slices).  forward -> a
    namedtuple of the five tapped maps.  `pretrained` is accepted for the reference's signature; PNet loads the weights (module
    docstring)."""

    def __init__(self, requires_grad=False, pretrained=True):
        super().__init__(_CFG, SLICES, requires_grad)

    def forward(self, X):
        return _Taps(*super().forward(X))


def default_weights_path():
    """Where torchvision caches its VGG16 checkpoint: torch.hub.get_dir()/checkpoints/vgg16-397923af.pth (TORCH_HOME decides)."""
    return vgg.default_weights_path(VGG16_FILE)


def vgg16_slices_state_dict(sd):
    """A torchvision VGG16 state dict (features.*; classifier.* ignored) or a PNet / vgg16 one -> vgg16's keys (slice1.0.weight, ...);
    KeyError for every features.N that is no convolution of VGG16."""
    return vgg.slices_state_dict(sd, "VGG16", CONVS, SLICES, own_prefix="net.")


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
            weights = vgg.cached_weights("PNet", "VGG16", VGG16_FILE)
        if weights is not None:
            self.load_weights(weights)
        self.L = self.net.N_slices
        if use_gpu:
            self.cuda()

    def load_weights(self, weights):
        """weights: a path (torch.load on the CPU, tensors only) or a state dict, in torchvision's or PNet's format."""
        self.net.load_state_dict(vgg16_slices_state_dict(vgg.load(weights)))

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
        """The 13 convolutions prepared for the kernels (vgg.prepare_convs: w0, b0, packed), once per set of weights and device
        (routing.cached); None when fp16 cannot hold a weight (torch then runs)."""
        convs = self.net.convs()
        return cached(self, f"_hip_cache_{device}", [t for c in convs for t in (c.weight, c.bias)],
                      lambda: vgg.prepare_convs(convs, device))

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
