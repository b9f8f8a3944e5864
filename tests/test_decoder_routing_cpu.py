"""CPU-only: what decides which kernel a layer of the refinement decoder gets (networks/routing.py, networks/conv_routes.py): the four route
switches, one behaviour checked on each, and the test of a plain convolution over a table of modules that must and must not be taken
apart."""
import os
import types

import pytest
import torch
import torch.nn as nn

from pixelsynth_amd.networks import architectures as A, block_train as BT, conv_routes as C, f16x3, norm_train as NT
from pixelsynth_amd.networks.routing import Switch

# (switch, the module whose global is the process default, that global, the variable, default, the other value, option attribute, the
# module's own name for resolve)
SWITCHES = {
    "decoder_conv": (f16x3.decoder_conv, A, "DECODER_CONV", "PS_DECODER_CONV", "f16x3", "fp32", "decoder_conv", lambda *a: A._conv_mode(*a)),
    "decoder_conv_train": (f16x3.decoder_conv_train, f16x3, "DECODER_CONV_TRAIN", "PS_DECODER_CONV_TRAIN", "fp32", "f16x3", "decoder_conv_train",
                           lambda *a: f16x3.train_mode(*a)),
    "decoder_norm_train": (NT.decoder_norm_train, NT, "DECODER_NORM_TRAIN", "PS_DECODER_NORM_TRAIN", "hip", "torch", None, lambda *a: NT.mode(*a)),
    "decoder_block_train": (BT.decoder_block_train, BT, "DECODER_BLOCK_TRAIN", "PS_DECODER_BLOCK_TRAIN", "torch", "hip", "decoder_block_train",
                            lambda *a: BT.mode(*a)),
}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_the_switch(name, monkeypatch):
    """Every switch: the default from an empty mapping and from one that sets the variable; the module global read at import and again at
    every call; the options over the process default where the switch has an option; with blocks over both, nesting, and the stack
    restored when the block raises; ValueError for an unknown mode in the constructor and, naming the variable, for a process default or
    an option outside the allowed values."""
    sw, home, var, env, default, other, attr, mode = SWITCHES[name]
    assert isinstance(sw, Switch) and getattr(A, name) is sw and sw.name == name and set(sw.values) == {default, other}
    assert sw.from_env({}) == default and sw.from_env({env: other}) == other
    assert getattr(home, var) == os.environ.get(env, default)
    monkeypatch.setattr(home, var, sw.from_env({}))
    assert mode() == default and mode(object()) == default and mode(types.SimpleNamespace()) == default and sw.forced() is None
    ask_other = types.SimpleNamespace(**{attr or name: other})
    ask_default = types.SimpleNamespace(**{attr or name: default})
    with_opt = other if attr else default                          # (a switch without an option ignores the options)
    assert mode(ask_other) == with_opt
    monkeypatch.setattr(home, var, other)                          # the global is read at every call
    assert mode() == other and mode(ask_default) == (default if attr else other)
    with sw(default) as block:                                     # the block over both
        assert block.mode == default and mode() == default and mode(ask_other) == default and sw.forced() == default
        with getattr(A, name)(other):
            assert mode() == other and mode(ask_default) == other and sw.forced() == other
        assert mode(ask_other) == default and sw.forced() == default
    assert mode() == other and sw.forced() is None
    with pytest.raises(KeyError):                                  # an exception inside leaves the stack as it was
        with sw(default):
            with sw(other):
                raise KeyError(name)
    assert mode() == other and sw.forced() is None
    with pytest.raises(ValueError, match=f"{name}: '{sw.values[0]}' or '{sw.values[1]}'"):
        sw("fast")
    assert sw.forced() is None
    monkeypatch.setattr(home, var, "fast")
    with pytest.raises(ValueError, match=env):
        mode()
    with sw(default):                                              # (a block in effect is what holds, whatever the default says)
        assert mode() == default
    monkeypatch.setattr(home, var, default)
    if attr:
        with pytest.raises(ValueError, match=env):
            mode(types.SimpleNamespace(**{attr: "fast"}))
    assert mode() == default


class _SubConv(nn.Conv2d):
    pass


def _hooked():
    conv = nn.Conv2d(8, 8, 3, 1, 1)
    conv.register_forward_hook(lambda mod, args, out: out + 1)
    return conv


# (a module, the k and padding it is asked as, whether plain_conv takes it, whether _plain_conv_weight hands out its weight)
CONVS = {
    "plain 3x3": (lambda: nn.Conv2d(8, 8, 3, 1, 1), 3, 1, True, True),
    "plain 1x1": (lambda: nn.Conv2d(8, 8, 1), 1, 0, True, True),
    "legacy spectral norm": (lambda: nn.utils.spectral_norm(nn.Conv2d(8, 8, 3, 1, 1)), 3, 1, True, True),
    "3x3 asked as 1x1": (lambda: nn.Conv2d(8, 8, 3, 1, 1), 1, 0, False, True),
    "1x1 with padding": (lambda: nn.Conv2d(8, 8, 1, 1, 1), 1, 0, False, True),
    "stride 2": (lambda: nn.Conv2d(8, 8, 3, 2, 1), 3, 1, False, True),
    "dilation 2": (lambda: nn.Conv2d(8, 8, 3, 1, 1, dilation=2), 3, 1, False, True),
    "groups 2": (lambda: nn.Conv2d(8, 8, 3, 1, 1, groups=2), 3, 1, False, True),
    "reflect padding": (lambda: nn.Conv2d(8, 8, 3, 1, 1, padding_mode="reflect"), 3, 1, True, False),
    "subclass": (lambda: _SubConv(8, 8, 3, 1, 1), 3, 1, False, False),
    "forward hook": (_hooked, 3, 1, True, False),
    "parametrizations.spectral_norm": (lambda: nn.utils.parametrizations.spectral_norm(nn.Conv2d(8, 8, 3, 1, 1)), 3, 1, False, False),
}


@pytest.mark.parametrize("name", sorted(CONVS))
def test_which_convolutions_are_taken_apart(name):
    """plain_conv(conv, k, pad) is the geometry every kernel computes on exactly an nn.Conv2d; _plain_conv_weight hands out a weight only
    where running F.conv2d on it is what the module's forward does.  A route needs both, so each refused module fails at least one --
    and what fails both today (a subclass, the parametrizations API) was refused by _plain_conv_weight before plain_conv looked at the
    type."""
    make, k, pad, plain, apart = CONVS[name]
    torch.manual_seed(0)
    conv = make().eval()
    x = torch.randn(1, 8, 6, 6)
    with torch.no_grad():
        assert C.plain_conv(conv, k, pad) is plain
        weight = C._plain_conv_weight(conv, x)
        assert (weight is not None) is apart
        assert plain and apart or name not in ("plain 3x3", "plain 1x1", "legacy spectral norm")
        if plain and apart:      # taken apart: the weight is the one the module's forward uses
            assert torch.allclose(torch.nn.functional.conv2d(x, weight, conv.bias, 1, pad), conv(x), rtol=1e-6, atol=1e-6)
        # nothing on the host takes a route, and _conv_split is then the module's own forward, bias included
        assert C.conv1x1(conv, x) is None and C._thin_conv(conv, x) is None and C._f16x3_conv(conv, x) is None
        y, bias = C._conv_split(conv, x, "f16x3")
        assert bias is None and torch.equal(y, conv(x))
