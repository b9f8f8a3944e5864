"""The PercSim cases of tests/golden/percsim.npz and an fp64 restatement of the VGG16 perceptual similarity (torch float64 on the
CPU): standardise, the 13 convolutions with ReLU and 2 x 2 max-pools, and per tap 1 - the pixel mean of the cosine of the two images'
channel vectors, each divided by (its norm + 1e-10).  Shared by make_percsim_golden.py and the PercSim tests."""
import numpy as np
import torch
import torch.nn.functional as F

from pixelsynth_amd import synthetic as syn

WEIGHT_SEED = 7
# name, seed, B, H, W, mask kind (syn.metric_mask; with a mask the vis / invis variants are scored too)
CASES = [
    ("pairs_256", 11, 2, 256, 256, "none"),
    ("pair_512x256", 12, 1, 512, 256, "none"),
    ("masked_256", 13, 1, 256, 256, "ragged"),
    ("odd_96x160", 14, 2, 96, 160, "none"),
]
VARIANTS = ("plain", "vis", "invis")
SHIFT = np.array([-0.030, -0.088, -0.188], np.float32)    # the fp32 values PNet holds
SCALE = np.array([0.458, 0.448, 0.450], np.float32)
_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
_TAP_AFTER = (2, 7, 14, 21, 28)                             # the convolution whose ReLU is tapped
_POOL_AFTER = (2, 7, 14, 21)


def case_inputs(case):
    """-> (img1, img2) (B, 3, H, W) float32 in [0, 1], mask (B, 1, H, W) f32 or None"""
    name, seed, B, H, W, mkind = case
    a, b = syn.metric_pair(seed, B, 3, H, W, "noise_blur")
    return a, b, syn.metric_mask(mkind, seed + 100, B, H, W)


def variants(img1, img2, mask):
    """-> [(x0, x1)] of the scored variants, in [0, 1] as float32 (the masked images formed in fp32, as the callers form them)"""
    out = [(img1, img2)]
    if mask is not None:
        inv = (np.float32(1) - mask).astype(np.float32)
        out += [((img1 * mask).astype(np.float32), (img2 * mask).astype(np.float32)),
                ((img1 * inv).astype(np.float32), (img2 * inv).astype(np.float32))]
    return out


def _features64(x, sd):
    taps = []
    for i in _CONVS:
        x = F.relu(F.conv2d(x, torch.from_numpy(sd[f"features.{i}.weight"]).double(),
                            torch.from_numpy(sd[f"features.{i}.bias"]).double(), padding=1))
        if i in _TAP_AFTER:
            taps.append(x)
        if i in _POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return taps


def _score64(f0, f1):
    u = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    v = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return 1.0 - (u * v).sum(1).mean((1, 2))


def percsim64(x0, x1, sd):
    """x0, x1 (B, 3, H, W) float32 in [0, 1] -> (B, 6) float64: the five per-tap scores and their sum."""
    def prep(x):
        t = torch.from_numpy(np.ascontiguousarray(x)).double() * 2 - 1
        return (t - torch.from_numpy(SHIFT).double().view(1, 3, 1, 1)) / torch.from_numpy(SCALE).double().view(1, 3, 1, 1)
    with torch.no_grad():
        s = [_score64(a, b) for a, b in zip(_features64(prep(x0), sd), _features64(prep(x1), sd))]
    out = torch.stack(s, 1)
    return torch.cat([out, out.sum(1, keepdim=True)], 1).numpy()


def case64(case, sd=None):
    """-> (V, B, 6) float64 for the case's variants"""
    sd = syn.vgg16_state_dict(WEIGHT_SEED) if sd is None else sd
    return np.stack([percsim64(x0, x1, sd) for x0, x1 in variants(*case_inputs(case))])
