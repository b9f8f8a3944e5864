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

The trunk -- the features builder, the slices, the key translation, the loading and the preparation of the convolutions -- is
networks/vgg.py's, shared with PercSim's vgg16; here are VGG19's tables.
"""
from . import vgg
from .routing import cached

VGG19_FILE = "vgg19-dcbb9e9d.pth"    # torchvision's name of its VGG19 checkpoint
# torchvision's vgg19().features (configuration "E") up to relu5_1: 30 modules
_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512)
CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)    # the indices of the 13 convolutions in features
POOLS = (4, 9, 18, 27)
SLICES = ((0, 2), (2, 7), (7, 12), (12, 21), (21, 30))      # slice1 .. slice5 = features[lo:hi], each ends at its relu*_1
TAPS = ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "relu5_1")
TAPPED = (0, 2, 4, 8, 12)            # which of the 13 convolutions (counted 0 .. 12) feed a tap
POOL_BEFORE = (2, 4, 8, 12)          # which of them read a max-pooled map


def default_weights_path():
    """Where torchvision caches its VGG19 checkpoint: torch.hub.get_dir()/checkpoints/vgg19-dcbb9e9d.pth (TORCH_HOME decides)."""
    return vgg.default_weights_path(VGG19_FILE)


def vgg19_slices_state_dict(sd):
    """A torchvision VGG19 state dict (features.*; features.30 and later and classifier.* ignored) or a VGG19 one -> VGG19's keys;
    KeyError for a features.N below 30 that is no convolution of VGG19."""
    return vgg.slices_state_dict(sd, "VGG19", CONVS, SLICES, ignore_after=True)


class VGG19(vgg.Slices):
    """VGG19's features up to relu5_1 (module docstring); forward -> the list of the five tapped maps.  requires_grad=False freezes the
    parameters, as the reference does for its loss."""

    def __init__(self, requires_grad=False, weights=None, rand=False):
        super().__init__(_CFG, SLICES, requires_grad)
        if weights is None and not rand:
            weights = vgg.cached_weights("VGG19", "VGG19", VGG19_FILE)
        if weights is not None:
            self.load_weights(weights)

    def load_weights(self, weights):
        """weights: a path (torch.load on the CPU, tensors only) or a state dict, in torchvision's or VGG19's format."""
        self.load_state_dict(vgg19_slices_state_dict(vgg.load(weights)))

    def hip_layers(self, device):
        """The 13 convolutions prepared for the kernels, forward and backward (vgg.prepare_convs: w0, b0, packed, flipped, w0_flipped),
        once per set of weights and device (routing.cached); None when fp16 cannot hold a weight (torch then runs)."""
        convs = self.convs()
        return cached(self, f"_hip_cache_{device}", [t for c in convs for t in (c.weight, c.bias)],
                      lambda: vgg.prepare_convs(convs, device, backward=True))
