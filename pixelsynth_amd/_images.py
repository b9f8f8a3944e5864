"""What the front ends of the kernels that read strided image batches share (image_metrics.py, perceptual.py, consistency.py, fid.py):
the dtype codes, the stride array, the argument checks made before the first launch, the workspace and the cut into launches.
Every check raises before anything is queued; a CPU tensor is an error (no CPU fallback)."""
import ctypes

import torch

from . import _lib

DTYPES = {torch.float32: 0, torch.uint8: 1}      # PS_DTYPE_F32, PS_DTYPE_U8
MAX_B = 65535                                    # images of one launch (a grid dimension)
# what a mask's dtype may be: (as the error names it, the test)
FLOAT_OR_BOOL = ("floating point or bool", lambda d: d.is_floating_point or d == torch.bool)      # converted to float32 by the caller
CODED = ("float32 or uint8", lambda d: d in DTYPES)                                               # read in place by the kernel


def strides(t):
    """The element strides of a 4-D tensor as the int64[4] the entry points take"""
    return (ctypes.c_int64 * 4)(*t.stride())


def check_images(images, channels, layout):
    """images {name: tensor}, one batch or two of one shape and dtype; channels: the C accepted; layout: how the error spells the
    shape, "(B, C, H, W)" -> (B, C, H, W)"""
    for name, t in images.items():
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor")
        if t.dim() != 4:
            raise ValueError(f"{name} must be {layout}, got shape {tuple(t.shape)}")
    names, (first, *others) = " and ".join(images), images.values()
    for t in others:
        if t.shape != first.shape:
            raise ValueError(f"{names} differ in shape: {tuple(first.shape)} vs {tuple(t.shape)}")
    B, C, H, W = first.shape
    if C not in channels:
        raise ValueError(f"C must be {' or '.join(map(str, channels))}, got {C}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"empty image batch {tuple(first.shape)}")
    if any(t.dtype != first.dtype for t in others) or first.dtype not in DTYPES:
        if others:
            raise TypeError(f"{names} must both be float32 or both uint8, got {' and '.join(str(t.dtype) for t in images.values())}")
        raise TypeError(f"{names} must be float32 or uint8, got {first.dtype}")
    return B, C, H, W


def check_mask(name, mask, shape, kinds):
    """mask: a tensor of `shape` = (B, 1, H, W) whose dtype is one of `kinds` (FLOAT_OR_BOOL, CODED)"""
    if not torch.is_tensor(mask) or tuple(mask.shape) != shape:
        raise ValueError(f"{name} must be (B, 1, H, W) = {shape}, got {tuple(getattr(mask, 'shape', ()))}")
    if not kinds[1](mask.dtype):
        raise TypeError(f"{name} must be {kinds[0]}, got {mask.dtype}")


def same_device(**tensors):
    """The named tensors (None: an argument not given) are on one ROCm device -> that device"""
    given = [t for t in tensors.values() if t is not None]
    _lib.require_cuda(*given)
    devs = {t.device for t in given}
    if len(devs) != 1:
        names = list(tensors)
        raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} must be on one device, got {sorted(map(str, devs))}")
    return given[0].device


def workspace(entry, *dims, device):
    """-> (a workspace of the size the query `entry` gives for dims, that size)"""
    nbytes = _lib.call(entry, *dims)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def batches(B, per=MAX_B):
    """(b0, b1) of the launches over B images, `per` at most each"""
    return ((b0, min(B, b0 + per)) for b0 in range(0, B, per))
