"""GPU: the per-module cache of a derived weight behind the decoder's three cached routes (networks/conv_routes.py: cached) follows the
weight, and a convolution that must not be taken apart runs whole."""
import pytest
import torch
import torch.nn as nn

from pixelsynth_amd.networks import architectures as A, conv_routes as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last

# route -> (Ci, Co, k, shape of x, the call, its cache slot): each at the smallest shape its own size test accepts
ROUTES = {
    "1x1": (32, 64, 1, (1, 32, 4, 4), lambda conv, x: C.conv1x1(conv, x), "_ps_1x1_cache"),
    "thin-in": (4, 64, 3, (1, 4, 8, 16), lambda conv, x: C._thin_conv(conv, x), "_ps_thin_cache"),
    "thin-out": (32, 3, 3, (1, 32, 8, 32), lambda conv, x: C._thin_conv(conv, x), "_ps_thin_cache"),
    "f16x3": (32, 64, 3, (1, 32, 16, 16), lambda conv, x: A._f16x3_conv(conv, x), "_ps_f16x3_cache"),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_cached_weight_follows_the_weight(route):
    """Run; write to the weight in place (its version counter moves); replace its storage (its address moves): every time the route gives
    the bits a fresh module with the same weight gives, and other bits than before.  Two runs with nothing changed in between do not
    derive the weight again: the cache entry holds the same object."""
    Ci, Co, k, shape, run, slot = ROUTES[route]
    g = torch.Generator().manual_seed(3)
    conv = nn.Conv2d(Ci, Co, k, 1, k // 2).to(DEV).eval()
    x = torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=CL)

    def fresh():
        other = nn.Conv2d(Ci, Co, k, 1, k // 2).to(DEV).eval()
        other.load_state_dict(conv.state_dict())
        assert slot not in other.__dict__ and other.weight.data_ptr() != conv.weight.data_ptr()
        return run(other, x)
    with torch.no_grad():
        first = run(conv, x)
        assert first is not None and first.shape == (shape[0], Co) + shape[2:] and torch.equal(first, fresh())
        held = conv.__dict__[slot][1]
        again = run(conv, x)
        assert conv.__dict__[slot][1] is held and held is not None and torch.equal(again, first)
        conv.weight.mul_(1.5)                                   # in place: the same address, another version
        second = run(conv, x)
        assert conv.__dict__[slot][1] is not held and torch.equal(second, fresh()) and not torch.equal(second, first)
        held = conv.__dict__[slot][1]
        conv.weight.data = (torch.randn(conv.weight.shape, generator=g) * 0.1).to(DEV)     # another tensor: another address
        third = run(conv, x)
        assert conv.__dict__[slot][1] is not held and torch.equal(third, fresh()) and not torch.equal(third, second)
    A.check_f16x3_overflow(torch.device(DEV))


def test_a_convolution_that_cannot_be_taken_apart_runs_whole():
    """A 64 -> 64 3 x 3 convolution with a forward hook -- the split-fp16 kernel's own shape, refused by _plain_conv_weight -- on the
    no-grad route: no kernel of the package takes it, and _conv_split is conv(x) bit for bit, bias and hook included, the hook fired once."""
    torch.manual_seed(5)
    conv = nn.Conv2d(64, 64, 3, 1, 1).to(DEV).eval()
    fired = []
    conv.register_forward_hook(lambda mod, args, out: (fired.append(out + 1), fired[-1])[1])
    x = torch.randn(1, 64, 16, 16, device=DEV).contiguous(memory_format=CL)
    with torch.no_grad():
        assert C._f16x3_takes(conv, x)
        assert A._f16x3_conv(conv, x) is None and C._thin_conv(conv, x) is None and C.conv1x1(conv, x) is None and not fired
        y, bias = C._conv_split(conv, x, "f16x3")
        # MIOpen's answers to this shape differ in the last bit from call to call, so conv(x) "bit for bit" is the very tensor that the
        # one call of the module returned -- the hook's -- and that tensor is the convolution, bias and the hook's + 1 included
        assert len(fired) == 1 and bias is None and y is fired[0]
        ref = torch.nn.functional.conv2d(x.double().cpu(), conv.weight.double().cpu(), conv.bias.double().cpu(), 1, 1) + 1
    # (64 * 9 products summed in fp32, each step within 2^-24 of the output's scale: far below the bias, about 0.02, or the hook's 1)
    assert (y.double().cpu() - ref).abs().max().item() <= 64 * 9 * 2.0 ** -24 * ref.abs().max().item()
    assert not any(k.startswith("_ps_") for k in conv.__dict__)
