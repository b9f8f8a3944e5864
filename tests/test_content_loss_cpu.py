"""CPU-only: the host side of the VGG19 content loss (csrc/content_loss.hip, networks/vgg19.py, losses/synthesis.py): the C ABI of
libpixelsynth_content.so against its header and bindings, VGG19's structure and weight conventions, the torch route of PerceptualLoss
against the formula written out in tests/_content_loss_ref.py, SynthesisLoss's dict, and the aliases.  Every test fails on the parent
commit: the modules do not exist.  The tensors go where SynthesisLoss puts its terms (the device when there is one)."""
import os
import re
import subprocess
import sys
import types

import pytest
import torch
import torch.nn as nn

import _content_loss_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, compat
from pixelsynth_amd.losses import synthesis as S
from pixelsynth_amd.networks import architectures as A, vgg19 as V


def test_the_registry_has_the_content_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "content")
    assert entry.so == "libpixelsynth_content.so" and entry.headers == ("pixelsynth_content.h",)
    assert entry.last_error == "ps_content_last_error"
    assert [u for u, _ in entry.units] == ["content_loss.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("content")
    assert set(protos) == set(_lib.CONTENT_PROTOS) == {
        "ps_content_last_error", "ps_content_tiles", "ps_content_input", "ps_content_bias", "ps_content_tap", "ps_content_finish",
        "ps_content_pool", "ps_content_join"}
    assert _lib.PROTOS["content"] is _lib.CONTENT_PROTOS and [e.name for e in _libraries.LIBRARIES] == list(_lib.PROTOS)
    header = open(os.path.join(ROOT, "include", "pixelsynth_content.h")).read()
    tile = int(re.search(r"#define PS_CONTENT_TILE (\d+)", header).group(1))
    assert tile == 256 and int(re.search(r"#define PS_CONTENT_THREADS (\d+)", header).group(1)) == 256
    assert int(re.search(r"#define PS_CONTENT_LEVELS (\d+)", header).group(1)) == 5
    for npix in (1, 255, 256, 257, 3 * 6 * 10, 16 * 256 * 256, 2 ** 33 + 1):
        assert _lib.call("ps_content_tiles", npix) == -(-npix // tile)
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)


def test_the_entry_points_refuse_before_a_launch():
    """Host-side refusals: nothing is queued, so plain host memory stands in for the buffers"""
    L = _lib.library("content")
    buf = torch.zeros(64, dtype=torch.float64)
    p = buf.data_ptr()
    assert p % 16 == 0
    for rc in (L.ps_content_tap(p, 1, 2, 2, 32, p, None), L.ps_content_tap(p + 4, 1, 2, 2, 64, p, None), L.ps_content_tap(None, 1, 2, 2, 64, p, None),
               L.ps_content_pool(p, 1, 3, 2, 64, p, None), L.ps_content_bias(p, p, 0, 64, None),
               L.ps_content_join(p, None, None, None, None, 1.0, 1, 2, 2, 64, 0, p + 4096, None),        # neither term
               L.ps_content_join(p, None, p, None, None, 1.0, 1, 2, 2, 64, 0, p + 4096, None),           # up without its scale
               L.ps_content_join(p, p, None, None, p, 1.0, 1, 2, 2, 64, 1, p + 4096, None),              # a pool without up
               L.ps_content_join(p, p, None, None, p, 1.0, 1, 2, 2, 64, 0, p, None),                     # in place
               L.ps_content_join(p, p, p, p, p, 1.0, 1, 3, 2, 64, 1, p + 4096, None)):
        assert rc != 0 and L.ps_content_last_error()
    strides = (torch.tensor([1, 1, 1, -1], dtype=torch.int64), torch.tensor([1, 1, 1, 1], dtype=torch.int64))
    assert L.ps_content_input(p, strides[0].data_ptr(), p, strides[1].data_ptr(), 1, 2, 2, p, None) != 0
    assert L.ps_content_input(p, strides[1].data_ptr(), p, strides[1].data_ptr(), 0, 2, 2, p, None) != 0


def test_vgg19_has_torchvisions_structure_and_names():
    torch.manual_seed(0)
    net = A.VGG19(rand=True)
    assert A.VGG19 is V.VGG19 and list(net.state_dict()) == ref.KEYS
    assert not any(p.requires_grad for p in net.parameters()) and all(p.requires_grad for p in V.VGG19(requires_grad=True, rand=True).parameters())
    want = []
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512):
        want += ["M"] if v == "M" else [v, "R"]
    assert len(want) == 30
    for s, (lo, hi) in enumerate(((0, 2), (2, 7), (7, 12), (12, 21), (21, 30))):
        sl = getattr(net, f"slice{s + 1}")
        assert [n for n, _ in sl.named_children()] == [str(i) for i in range(lo, hi)]
        for i, m in zip(range(lo, hi), sl):
            if want[i] == "M":
                assert isinstance(m, nn.MaxPool2d) and m.kernel_size == 2 and m.stride == 2 and i in ref.POOLS
            elif want[i] == "R":
                assert isinstance(m, nn.ReLU)
            else:
                assert isinstance(m, nn.Conv2d) and m.out_channels == want[i] and m.kernel_size == (3, 3) and m.padding == (1, 1) and i in ref.CONVS
    assert [c.out_channels for c in net.convs()] == list(ref.WIDTHS) and float(net.convs()[3].bias.abs().max()) == 0.0
    x = torch.randn(1, 3, 32, 32)
    out = net(x)
    assert isinstance(out, list) and [tuple(t.shape[1:]) for t in out] == [(64, 32, 32), (128, 16, 16), (256, 8, 8), (512, 4, 4), (512, 2, 2)]
    for got, want_t in zip(out, ref.features(net.state_dict(), x)):     # the input is used as it comes
        assert torch.equal(got, want_t)


def test_vgg19_loads_both_key_formats_and_downloads_nothing(tmp_path, monkeypatch):
    torch.manual_seed(1)
    src = V.VGG19(rand=True)
    own = {k: v.clone() for k, v in src.state_dict().items()}
    tv = {f"features.{k.split('.', 1)[1]}": v for k, v in own.items()}
    tv.update({"features.30.weight": torch.zeros(1), "features.34.bias": torch.zeros(1), "classifier.0.weight": torch.zeros(2, 2)})
    path = tmp_path / "vgg19.pth"
    torch.save(tv, path)
    for weights in (own, tv, str(path)):
        net = V.VGG19(weights=weights)
        assert all(torch.equal(net.state_dict()[k], own[k]) for k in ref.KEYS)
    with pytest.raises(KeyError):
        V.VGG19(weights={**tv, "features.3.weight": torch.zeros(1)})
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "nothing_here"))
    assert V.default_weights_path() == os.path.join(str(tmp_path / "nothing_here"), "hub", "checkpoints", "vgg19-dcbb9e9d.pth")
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        V.VGG19()
    with pytest.raises(FileNotFoundError):
        S.PerceptualLoss(types.SimpleNamespace())


def _pair(seed, P, size, dev="cpu"):
    gen = torch.Generator().manual_seed(seed)
    return torch.tanh(torch.randn(P, 3, size, size, generator=gen)).to(dev), torch.tanh(torch.randn(P, 3, size, size, generator=gen)).to(dev)


def test_the_torch_route_is_the_written_out_formula():
    torch.manual_seed(2)
    term = S.PerceptualLoss(None, rand=True)
    with torch.no_grad():
        for c in term.model.convs():
            c.bias.normal_(0, 0.1)
    assert term.weights == list(ref.WEIGHTS) and isinstance(term.criterion, nn.L1Loss)
    pred, gt = _pair(3, 2, 32)
    pred.requires_grad_()
    out = term(pred, gt)
    assert set(out) == {"Perceptual", "Total Loss"} and out["Perceptual"] is out["Total Loss"]
    sd = term.model.state_dict()
    want, want_levels = ref.loss(sd, pred, gt)
    total, levels, saved = S.content_loss(term.model, pred, gt, return_saved=True)
    assert saved is None and not S.hip_takes(term.model, pred, gt)
    assert torch.equal(out["Total Loss"], want) and torch.equal(total, want) and torch.equal(levels, torch.stack(want_levels))
    assert not levels.requires_grad
    want64, _ = ref.loss(ref.cast(sd, torch.float64), pred.double(), gt.double())
    rel = abs(want.item() - want64.item()) / want64.item()
    print(f"fp32 torch route against the fp64 formula: relative error {rel:.3e} / 1e-6")
    assert rel <= 1e-6
    g, = torch.autograd.grad(out["Total Loss"], pred)
    g_want, = torch.autograd.grad(want, pred)
    assert torch.equal(g, g_want) and float(g.abs().max()) > 0


def test_synthesis_loss_keeps_the_first_term_unweighted():
    torch.manual_seed(4)
    opt = types.SimpleNamespace(losses=["2.0_l1", "10.0_content"], vgg19_rand=True)
    crit = S.SynthesisLoss(opt)
    assert [type(m) for m in crit.losses] == [S.L1LossWrapper, S.PerceptualLoss, S.PSNR, S.SSIM] and crit.lambdas == [2.0, 10.0]
    assert all(m is not None for m in crit.losses)           # (the reference hands back None where there is no device)
    dev = next(crit.parameters()).device
    assert dev.type == ("cuda" if torch.cuda.is_available() else "cpu")
    pred, gt = _pair(5, 2, 32, dev)
    pred.requires_grad_()
    out = crit(pred, gt)
    assert set(out) == {"L1", "Perceptual", "Total Loss", "psnr", "ssim"}
    l1 = (pred - gt).abs().mean()
    assert torch.equal(out["L1"], l1) and torch.equal(out["Total Loss"], out["L1"] + out["Perceptual"] * 10.0)      # not 2 L1 + ...
    mse = (pred - gt).pow(2).sum(1).view(2, -1).mean(1)
    assert torch.equal(out["psnr"], (10 * (1 / mse).log10()).mean().detach()) and not out["psnr"].requires_grad
    assert out["ssim"].dim() == 0 and not out["ssim"].requires_grad and -1.0 <= float(out["ssim"]) <= 1.0
    out["Total Loss"].backward()
    assert pred.grad is not None and bool(torch.isfinite(pred.grad).all()) and float(pred.grad.abs().max()) > 0
    # a single content term is taken as it is, whatever its lambda; an unknown name is an error
    alone = S.SynthesisLoss(types.SimpleNamespace(losses=["10.0_content"], vgg19_rand=True))
    alone.losses[0] = crit.losses[1]
    single = alone(pred, gt)
    assert single["Total Loss"] is single["Perceptual"] and "L1" not in single
    with pytest.raises(ValueError):
        S.SynthesisLoss(types.SimpleNamespace(losses=["1.0_style"]))


def test_the_host_ssim_is_the_reference_formula_in_fp64():
    pred, gt = _pair(6, 2, 24)
    got = S.SSIM()(pred, gt)["ssim"]
    a, b = pred.double(), gt.double()
    taps = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / 4.5)
    win = torch.outer(taps / taps.sum(), taps / taps.sum()).expand(3, 1, 11, 11).contiguous()
    blur = lambda t: torch.nn.functional.conv2d(t, win, padding=5, groups=3)
    m1, m2 = blur(a), blur(b)
    want = (((2 * m1 * m2 + 1e-4) * (2 * (blur(a * b) - m1 * m2) + 9e-4))
            / ((m1 * m1 + m2 * m2 + 1e-4) * (blur(a * a) - m1 * m1 + blur(b * b) - m2 * m2 + 9e-4))).mean()
    print(f"host SSIM against fp64: {abs(got.item() - want.item()):.3e} / 1e-5")
    assert abs(got.item() - want.item()) <= 1e-5


def test_the_training_aliases_install_and_leave_the_other_tables_alone():
    assert compat.TRAINING_ALIASES == {"models.losses.synthesis": "pixelsynth_amd.losses.synthesis"}
    assert len(compat.ALIASES) == 9 and "models.losses.synthesis" not in compat.ALIASES
    assert compat.EVAL_ALIASES == {"evaluation.metrics": "pixelsynth_amd.evaluation.metrics", "models.losses.ssim": "pixelsynth_amd.losses.ssim"}
    code = ("import sys; import pixelsynth_amd.compat as c; before = set(sys.modules); got = c.install_training_aliases(); "
            "assert got == ['models.losses.synthesis'], got; "
            "from models.losses.synthesis import SynthesisLoss, PerceptualLoss, L1LossWrapper, PSNR, SSIM; "
            "import pixelsynth_amd.losses.synthesis as s; assert SynthesisLoss is s.SynthesisLoss and sys.modules['models.losses.synthesis'] is s; "
            "assert 'models.losses.ssim' not in sys.modules and 'evaluation.metrics' not in sys.modules and 'models.vqvae2.vqvae' not in sys.modules; "
            "assert c.install_training_aliases() == []; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env={**os.environ, "PYTHONPATH": ROOT})
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr
