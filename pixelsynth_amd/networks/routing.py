"""What the refinement decoder's routes share, so that each is decided in one place: the switch that names a route (decoder_conv,
decoder_conv_train, decoder_norm_train, decoder_block_train and decoder_thin_train are instances), the cache of what is prepared from a module's weights (cached), the test of
what the kernels accept as a tensor, and the three tensor idioms every route repeats.  Imports nothing of the package: every module of networks/ may import it."""
import os
import sys

import torch


class _Forced:
    """What switch(mode) returns: `mode` on the switch's stack for the duration of the with block"""

    def __init__(self, stack, mode):
        self._stack, self.mode = stack, mode

    def __enter__(self):
        self._stack.append(self.mode)
        return self

    def __exit__(self, *exc):
        self._stack.pop()
        return False


class Switch:
    """A route switch `name` with the allowed `values`.  `with switch(mode): ...` forces `mode` for the calls inside, whatever the options
    say; blocks nest, the innermost wins.  Outside any block resolve(opt) is opt.<attr>, where the switch has an option and it is set, else
    the process default: the global `var` of the module named `module`, which that module fills at import from the environment variable
    `env` (from_env) and which is read again at every call, so a caller or a test may assign it."""

    def __init__(self, name, env, values, default, module, var, attr=None):
        self.name, self.env, self.values, self.default, self.module, self.var, self.attr = name, env, values, default, module, var, attr
        self.expected = " or ".join(repr(v) for v in values)
        self._stack = []        # the modes forced, innermost last

    def from_env(self, environ=None):
        """`env` of the mapping `environ` (the process's environment): `default` unless set"""
        return (os.environ if environ is None else environ).get(self.env, self.default)

    def __call__(self, mode):
        if mode not in self.values:
            raise ValueError(f"{self.name}: {self.expected}")
        return _Forced(self._stack, mode)

    def forced(self):
        """The mode of the innermost block in effect, or None"""
        return self._stack[-1] if self._stack else None

    def resolve(self, opt=None):
        """The mode in effect for a caller whose options are `opt`.  ValueError for an option or a process default outside `values`: a
        misspelt variable must not quietly select the other route."""
        if self._stack:
            return self._stack[-1]
        mode = (self.attr and getattr(opt, self.attr, None)) or getattr(sys.modules[self.module], self.var)
        if mode not in self.values:
            raise ValueError(f"{self.name} / {self.env} = {mode!r}: {self.expected}")
        return mode


def cached(mod, slot, sources, make):
    """make() -- a value derived from the tensors `sources` of `mod` -- computed once and kept in mod.__dict__[slot] as (key, value, sources)
    until a source is replaced or written to (its address, version counter or device).  The sources are kept alive: their addresses are
    the key.  Every prepared weight of the package is kept this way: the decoder's (conv_routes.py), the VGG trunks' and the FID
    network's (hip_layers)."""
    key = tuple((t.data_ptr(), t._version, t.device) for t in sources)
    entry = mod.__dict__.get(slot)
    if entry is None or entry[0] != key:
        entry = mod.__dict__[slot] = (key, make(), sources)
    return entry[1]


PENDING = "_ps_sn_pending"    # mod.__dict__ slot of a spectral-normalised weight computed ahead of the module's call (spectral_train.py)


def _sn_versions(mod):
    return tuple((t.data_ptr(), t._version) for t in (mod.weight_orig, mod.weight_u, mod.weight_v))


def leave_pending(mod, weight):
    """Leave `weight` -- weight_orig / sigma as the batched pass computed it -- for the module's next request of its weight"""
    mod.__dict__[PENDING] = (weight, _sn_versions(mod))


def has_pending(mod):
    return PENDING in mod.__dict__


def take_pending(mod):
    """The weight left pending on `mod`, once: it is removed.  None where nothing is pending, or where weight_orig / u / v were replaced
    or written to since (an optimiser step, the hook itself): a weight of another state is dropped, not used."""
    entry = mod.__dict__.pop(PENDING, None)
    if entry is None or entry[1] != _sn_versions(mod):
        return None
    return entry[0]


def gpu_f32(t, layout=torch.channels_last, multiple=1, aligned=False, dims=4):
    """Whether `t` is a tensor the kernels take by raw pointer: on the GPU, fp32, of `dims` dimensions (None: any), dense in `layout`
    (None: any storage), size(1) a multiple of `multiple`, and, where `aligned`, at an address that is a multiple of 16 bytes.  The
    entry points differ in what they ask: each caller states its own conditions here and they are not levelled."""
    return (t is not None and t.is_cuda and t.dtype == torch.float32 and (dims is None or t.dim() == dims)
            and (multiple == 1 or t.size(1) % multiple == 0) and (layout is None or t.is_contiguous(memory_format=layout))
            and (not aligned or t.data_ptr() % 16 == 0))


def empty_nhwc(B, C, H, W, like):
    """An uninitialised (B, C, H, W) tensor in channels-last storage, of the type and on the device of `like`"""
    if C == 1:   # (channels_last of one channel is ambiguous to torch; the kernels write (B, H, W, C))
        return torch.empty((B, H, W, C), dtype=like.dtype, device=like.device).permute(0, 3, 1, 2)
    return torch.empty((B, C, H, W), dtype=like.dtype, device=like.device, memory_format=torch.channels_last)


def per_sample(t, B, C):
    """A per-channel table given for the whole batch or per sample -- (C), (1, C, 1, 1), (B, C), (B, C, 1, 1) -- as contiguous (B, C)"""
    return t.reshape(-1, C).expand(B, C).contiguous()


def grad_nhwc(grad):
    """The gradient a backward pass receives as the kernels read it: fp32, channels-last (a sliced or expanded one: one copy)"""
    return grad.to(torch.float32).contiguous(memory_format=torch.channels_last)
