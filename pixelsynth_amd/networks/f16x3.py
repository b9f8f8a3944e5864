"""The split-fp16 3 x 3 convolution (csrc/conv_f16x3.hip) of the refinement decoder and the VQ-VAE: weight packing, the launch and the
overflow guard.  Every product is three fp16 MFMAs on split operands, so an activation beyond fp16's range (|v| > 65000, or not a number)
gives a wrong output and sets a per-device flag (csrc/conv_thin.hip's 4 -> 64 layer likewise).  checked(device, fn) reads it: the
outermost scope clears the flag (an earlier, unchecked pass's is not this pass's), runs fn, synchronises, and if the flag is set warns and
runs fn again under decoder_conv("fp32"), every convolution through torch.  Inner scopes do nothing, so a pass made of guarded calls is
checked once.  A scope must not enclose a collective: a rerun on one rank would run it twice.
"""
import warnings

import torch

from .. import _lib

_FORCED_CONV = []   # decoder_conv(mode) in effect, innermost last
_flags = {}         # str(device) -> int32 (1,) overflow flag
_open = set()       # str(device) of the guarded scopes open


def forced_mode():
    """The mode of the innermost decoder_conv(...) in effect, or None."""
    return _FORCED_CONV[-1] if _FORCED_CONV else None


class decoder_conv:
    """with decoder_conv("fp32"): ... -- every split-fp16 convolution inside (decoder and VQ-VAE) through torch (MIOpen fp32), whatever
    the options say: how checked() reruns a pass whose split-fp16 convolutions met an activation beyond fp16's range."""

    def __init__(self, mode):
        if mode not in ("f16x3", "fp32"):
            raise ValueError("decoder_conv: 'f16x3' or 'fp32'")
        self.mode = mode

    def __enter__(self):
        _FORCED_CONV.append(self.mode)
        return self

    def __exit__(self, *exc):
        _FORCED_CONV.pop()
        return False


def flag(device):
    """The overflow flag the kernels set on `device` (int32 (1,), zero when first asked for)."""
    key = str(device)
    if key not in _flags:
        _flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _flags[key]


def check_f16x3_overflow(device):
    """Synchronises.  Raises (and clears the flag) if a split-fp16 convolution met an activation beyond fp16's range since the flag was
    last cleared: its output is then wrong."""
    f = _flags.get(str(device))
    if f is not None and int(f.item()):
        f.zero_()
        raise RuntimeError("an activation beyond fp16's range (|v| > 65000, or not a number) reached a split-fp16 convolution; "
                           "PS_DECODER_CONV=fp32 (refinement decoder) / PS_VQVAE_CONV=fp32 (VQ-VAE) run everything through torch")


def checked(device, fn, check=True):
    """fn() as a guarded scope on `device` (module docstring).  check=False: a scope that nobody inside checks -- for a caller that checks
    later, or accepts the risk."""
    key = str(device)
    if key in _open:            # the outermost scope owns the check
        return fn()
    _open.add(key)
    try:
        if not check:
            return fn()
        if key in _flags:
            _flags[key].zero_()
        out = fn()
        try:
            check_f16x3_overflow(device)
        except RuntimeError as err:
            warnings.warn(f"{err}: run again in fp32")
            with decoder_conv("fp32"):
                out = fn()
        return out
    finally:
        _open.discard(key)


def pack3x3(weight, bias=None, s2d=False, d2s=False):
    """A (Co, Ci, 3, 3) fp32 CUDA weight (and (Co) bias) packed for conv3x3, Co padded to a multiple of 64 (the first `live` channels are
    the layer's); s2d / d2s: for a space-to-depth input (Ci / 4 a multiple of 32) / a depth-to-space output (Co / 4 a multiple of 64).
    ValueError for a shape the kernel does not take or a weight fp16 cannot hold (synchronises to find out): the caller goes through torch."""
    Co, Ci = weight.shape[:2]
    if Ci % 32 or (s2d and Ci % 128) or (d2s and Co % 256):
        raise ValueError(f"split-fp16 convolution: {Co} x {Ci} channels (s2d {s2d}, d2s {d2s})")
    Cop = -(-Co // 64) * 64
    if Cop != Co:
        weight = torch.cat([weight, weight.new_zeros(Cop - Co, Ci, 3, 3)])
    wl = weight.permute(0, 2, 3, 1).contiguous()       # (Co, 3, 3, Ci): no copy for a channels_last weight
    top = float(wl.abs().max())
    if not (top == top and top < 6.0e4):
        raise ValueError("split-fp16 convolution: a weight fp16 cannot hold")
    packed = torch.empty(_lib.call("ps_conv3x3_f16x3_packed_bytes", Cop, Ci), dtype=torch.uint8, device=weight.device)
    _lib.call("ps_conv3x3_f16x3_pack", wl, Cop, Ci, packed)
    if bias is not None:
        bias = torch.cat([bias, bias.new_zeros(Cop - Co)]).contiguous()
    return dict(packed=packed, Ci=Ci, Co=Cop, live=Co, bias=bias, s2d=s2d, d2s=d2s)


def conv3x3(x, p, scale=None, shift=None, bias=None, res=None):
    """conv3x3(act(x)) + bias + res (ps_conv3x3_f16x3_ex_nhwc) of a pack3x3 layer on x (B, Ci, H, W) channels_last fp32 -- (B, Ci / 4, 2 H,
    2 W) for s2d --, act(x) = max(x * scale - shift, 0) (scale / shift (B, Ci)) or x; bias (Co) defaults to the layer's, res is NHWC.
    -> y (B, Co, H, W) channels_last, (B, Co / 4, 2 H, 2 W) for d2s."""
    B, C, H, W = x.shape
    if p["s2d"]:
        C, H, W = 4 * C, H // 2, W // 2
    assert C == p["Ci"] and x.is_contiguous(memory_format=torch.channels_last)
    shape = (B, p["Co"] // 4, 2 * H, 2 * W) if p["d2s"] else (B, p["Co"], H, W)
    y = torch.empty(shape, dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bias = p["bias"] if bias is None else bias
    _lib.call("ps_conv3x3_f16x3_ex_nhwc", x, scale, shift, p["packed"], bias, res, B, H, W, C, p["Co"], p["live"], int(p["s2d"]),
              int(p["d2s"]), y, flag(x.device))
    return y
