"""GPU: when the packs that hip_layers(device) prepares from a network's weights are stale (networks/routing.cached, the one keyed
cache) -- for PNet, VGG19 and FIDInception: the identical object twice, another one after load_weights and after an in-place write to one
convolution's weight, and the HIP score then follows the new weights.  Smallest shapes of the HIP routes: one pair of 256 x 256 images,
two 299 x 299 images for the FID network; torchvision's initialisation (rand=True).

Bounds: PercSim against the torch formula in fp64 on the same weights with tests/test_percsim_gpu.py's BOUND_TAP / BOUND_TOTAL; the
content loss against the fp64 formula with tests/_content_loss_ref.py's rule, as tests/test_content_loss_gpu.py applies it.  The FID
features carry no bound here: they equal, bit for bit, those of a fresh network that loaded the written weights.  The write scales the
output channels of one convolution by 0.25 .. 4 (a common factor would leave a cosine where it was): on the CPU it moves the PercSim
total by 2.7e-2 and doubles the content loss, so a pack that stayed would miss either bound by orders of magnitude."""
import pytest
import torch

import _content_loss_ref as ref
import fid_ref64
from pixelsynth_amd import fid, synthetic as syn
from pixelsynth_amd.losses import synthesis as S
from pixelsynth_amd.networks import f16x3
from pixelsynth_amd.networks.inception import FIDInception
from pixelsynth_amd.networks.pretrained_networks import PNet
from pixelsynth_amd.networks.vgg19 import VGG19
from test_percsim_gpu import BOUND_TAP, BOUND_TOTAL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _scale_channels(weight):
    with torch.no_grad():
        weight.mul_(torch.linspace(0.25, 4.0, weight.size(0), device=weight.device).view(-1, 1, 1, 1))


def _packs(net, load, write):
    """hip_layers twice, after load() and after write(): -> the three distinct objects"""
    first = net.hip_layers(DEV)
    assert first is not None and net.hip_layers(DEV) is first
    load()
    second = net.hip_layers(DEV)
    assert second is not None and second is not first and net.hip_layers(DEV) is second
    write()
    third = net.hip_layers(DEV)
    assert third is not None and third is not second and third is not first and net.hip_layers(DEV) is third
    return first, second, third


def test_percsim_follows_its_weights():
    torch.cuda.set_device(DEV)
    torch.manual_seed(5)
    net, other = PNet(pnet_rand=True, use_gpu=True), PNet(pnet_rand=True, use_gpu=False)
    a, b = syn.metric_pair(61, 1, 3, 256, 256)
    x0, x1 = torch.from_numpy(a).to(DEV) * 2 - 1, torch.from_numpy(b).to(DEV) * 2 - 1
    assert net.hip_takes(x0, x1)

    def check(what):
        with torch.no_grad():
            total, taps = net(x0, x1, retPerLayer=True)
            net64 = PNet(pnet_rand=True, use_gpu=False, weights=net.state_dict()).double().to(DEV)
            want, want_taps = net64.torch_forward(x0.double(), x1.double(), retPerLayer=True)
        d_taps = max((t.double() - w).abs().max().item() for t, w in zip(taps, want_taps))
        d_total = (total.double() - want).abs().max().item()
        print(f"percsim {what}: tap {d_taps:.3e} / {BOUND_TAP:.1e}, total {d_total:.3e} / {BOUND_TOTAL:.1e}")
        assert d_taps <= BOUND_TAP and d_total <= BOUND_TOTAL, what
        return total
    before = check("as built")
    _packs(net, lambda: net.load_weights(other.state_dict()), lambda: _scale_channels(net.net.convs()[1].weight))
    after = check("after load_weights and a write to conv1_2")
    assert abs(after.item() - before.item()) > 1e3 * BOUND_TOTAL


def test_content_loss_follows_its_weights():
    torch.cuda.set_device(DEV)
    torch.manual_seed(6)
    net, other = VGG19(rand=True).to(DEV), VGG19(rand=True)
    gen = torch.Generator().manual_seed(12)
    pred, gt = (torch.tanh(torch.randn(1, 3, 256, 256, generator=gen)).to(DEV) for _ in range(2))
    assert S.hip_takes(net, pred, gt)

    def check(what):
        with torch.no_grad():
            total, _ = S.content_loss(net, pred, gt)
            with f16x3.decoder_conv("fp32"):
                total32, _ = S.content_loss(net, pred, gt)
            total64, _ = ref.loss(ref.cast(net.state_dict(), torch.float64), pred.double(), gt.double())
        err, bound = ref.rule(f"content loss {what}", total, total64, total32)
        assert err <= bound, what
        return total
    before = check("as built")
    _packs(net, lambda: net.load_weights(other.state_dict()), lambda: _scale_channels(net.convs()[1].weight))
    after = check("after load_weights and a write to conv1_2")
    assert after.item() > 1.5 * before.item()


def test_fid_features_follow_their_weights():
    torch.cuda.set_device(DEV)
    t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    net = FIDInception(weights=t(fid_ref64.weights()), use_gpu=True)
    imgs = torch.from_numpy(syn.metric_pair(62, 2, 3, 299, 299)[0]).to(DEV)
    before = fid.inception_features(net, imgs)
    _packs(net, lambda: net.load_weights(t(fid_ref64.weights(fid_ref64.WEIGHT_SEED + 1))),
           lambda: _scale_channels(net.conv("Mixed_5b.branch1x1").conv.weight))
    after = fid.inception_features(net, imgs)
    fresh = FIDInception(weights={k: v.cpu() for k, v in net.state_dict().items()}, use_gpu=True)
    assert torch.equal(after, fid.inception_features(fresh, imgs)) and not torch.equal(after, before)
