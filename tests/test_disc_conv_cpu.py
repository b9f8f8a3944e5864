"""CPU: the discriminator's 4 x 4 convolution on the fp16 matrix pipe -- what needs no device: the registry entry and the header
against the prototype table, the switch, takes(), the torch route of conv4x4_train and of _SNConv, hip_routes_with_discriminator(), the
formulas of tests/_disc_conv_ref.py against fp64 autograd, and the Python mirror of the part plan against the header's formulas and the
library's answers."""
import argparse
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _disc_conv_ref as ref
import abi_util
from pixelsynth_amd import _lib, _libraries, training
from pixelsynth_amd.networks import disc_conv as DC
from pixelsynth_amd.networks.discriminators import _SNConv


# ---------------------------------------------------------------- registry and ABI
def test_registry_entry_sits_in_front_of_gan_train():
    names = [e.name for e in _libraries.LIBRARIES]
    assert names.index("disc_conv") == names.index("gan_train") - 1 and names[-1] == "gan_train"
    entry = _libraries.LIBRARIES[names.index("disc_conv")]
    assert entry.so == "libpixelsynth_disc_conv.so" and entry.last_error == "ps_disc_conv_last_error"
    assert [u for u, _ in entry.units] == ["disc_conv.hip"] and entry.headers == ("pixelsynth_disc_conv.h",)
    assert list(_lib.PROTOS).index("disc_conv") == list(_lib.PROTOS).index("gan_train") - 1
    assert _lib.PROTOS["disc_conv"] is _lib.DISC_CONV_PROTOS


def test_header_matches_the_prototype_table():
    protos = abi_util.assert_library_matches_header("disc_conv")
    assert set(protos) == {"ps_disc_conv_last_error", "ps_disc_conv_takes", "ps_disc_conv_workspace_bytes", "ps_disc_conv_parts",
                           "ps_disc_conv_forward_f16x3", "ps_disc_conv_backward_f16x3"}
    # the padding is an argument of the ABI
    assert all(any(re.fullmatch(r"int\s+pad", p) for p in protos[n]) for n in protos if n != "ps_disc_conv_last_error")


def test_main_library_exports_do_not_move():
    assert "ps_disc_conv_forward_f16x3" not in _lib.exported_symbols()


# ---------------------------------------------------------------- the switch
def test_switch_default_order_and_bad_value(monkeypatch):
    sw = DC.discriminator_conv_train
    assert sw.default == "torch" and sw.values == ("f16", "torch") and sw.env == "PS_DISCRIMINATOR_CONV_TRAIN"
    assert sw.from_env({}) == "torch" and sw.from_env({"PS_DISCRIMINATOR_CONV_TRAIN": "f16"}) == "f16"
    monkeypatch.setattr(DC, "DISCRIMINATOR_CONV_TRAIN", "torch")
    assert DC.mode() == "torch" and DC.mode(argparse.Namespace()) == "torch"
    opt = argparse.Namespace(discriminator_conv_train="f16")
    assert DC.mode(opt) == "f16"                                   # the options before the environment
    monkeypatch.setattr(DC, "DISCRIMINATOR_CONV_TRAIN", "f16")
    assert DC.mode() == "f16" and DC.mode(argparse.Namespace(discriminator_conv_train="torch")) == "torch"
    with sw("torch"):                                              # the call before the options
        assert DC.mode(opt) == "torch"
        with sw("f16"):
            assert DC.mode(argparse.Namespace(discriminator_conv_train="torch")) == "f16"
        assert DC.mode(opt) == "torch"
    with pytest.raises(ValueError):
        sw("hip")
    with pytest.raises(ValueError):
        DC.mode(argparse.Namespace(discriminator_conv_train="fp16"))
    monkeypatch.setattr(DC, "DISCRIMINATOR_CONV_TRAIN", "yes")
    with pytest.raises(ValueError):
        DC.mode()


# ---------------------------------------------------------------- takes
def test_takes_refuses_what_the_kernels_do_not_take():
    x, w = torch.zeros(1, 64, 5, 5), torch.zeros(64, 64, 4, 4)
    assert not DC.takes(x, w, 1)                                                                     # a CPU tensor
    ok = (2, 64, 128, 33, 34)
    assert DC.sizes_take(*ok, 1) and DC.sizes_take(*ok, 2) and DC.sizes_take(1, 512, 512, 1, 1, 1)
    assert not DC.sizes_take(*ok, 3) and not DC.sizes_take(*ok, 2, pad=1) and not DC.sizes_take(*ok, 0)
    assert not DC.sizes_take(2, 8, 64, 33, 34, 1) and not DC.sizes_take(2, 64, 96, 33, 34, 1) and not DC.sizes_take(2, 576, 64, 33, 34, 1)
    assert not DC.sizes_take(1, 512, 512, 4096, 4096, 1)                                             # a frame beyond 32-bit offsets
    # the layout and type conditions: everything takes() asks besides the device
    assert DC.operands_take(x, w)
    assert not DC.operands_take(x.to(memory_format=torch.channels_last), w) and not DC.takes(x.to(memory_format=torch.channels_last), w, 1)
    assert not DC.operands_take(x.double(), w.double()) and not DC.operands_take(x, w.double()) and not DC.takes(x.double(), w.double(), 1)
    assert not DC.operands_take(x, torch.zeros(64, 64, 3, 3)) and not DC.operands_take(x[:, :, :, ::2], w)


@pytest.mark.parametrize("shape", ref.ALL_SHAPES + [(32, 64, 128, 129, 129, 2), (32, 256, 512, 33, 33, 1), (32, 256, 512, 17, 18, 1)], ids=str)
def test_library_agrees_with_the_python_mirror(shape):
    B, Ci, Co, H, W, stride = shape
    assert _lib.call("ps_disc_conv_takes", B, Ci, Co, H, W, stride, 2) == 1 and DC.sizes_take(B, Ci, Co, H, W, stride)
    p = ref.plan(*shape)
    assert _lib.call("ps_disc_conv_parts", B, Ci, Co, H, W, stride, 2) == p.parts
    assert 1 <= p.parts <= ref.MAX_PARTS and p.chunk >= ref.MIN_CHUNK and (p.parts - 1) * p.chunk + p.last == p.steps
    # the header's formulas, spelt out
    assert p.steps == B * -(-(p.Ho * (p.Wo8 // 8)) // 2) and p.blocks == (Co // 64) * (Ci // 32)
    assert p.chunk == max(8, -(-p.steps // min(256, -(-512 // p.blocks))))
    assert _lib.call("ps_disc_conv_workspace_bytes", B, Ci, Co, H, W, stride, 2) > 16 * Co * Ci * 4
    for bad in ((B, Ci, Co, H, W, 3, 2), (B, Ci, Co, H, W, stride, 1), (B, 8, Co, H, W, stride, 2)):
        assert _lib.call("ps_disc_conv_takes", *bad) == 0 and _lib.call("ps_disc_conv_parts", *bad) == 0
        assert _lib.call("ps_disc_conv_workspace_bytes", *bad) == 0


def test_the_cases_reach_their_branches():
    plans = {s: ref.plan(*s) for s in ref.ALL_SHAPES}
    assert plans[(1, 64, 64, 1, 1, 1)].parts == 1 and plans[(1, 64, 64, 1, 1, 1)].steps == 1            # one step, one part
    p = plans[(3, 64, 64, 33, 34, 2)]
    assert p.parts == 10 and p.last == 6 and p.straddle == [3, 6] and p.odd_tail        # a shorter last part, parts in two frames, a zero chunk
    p = plans[(1, 64, 64, 33, 33, 1)]
    assert p.pixel_groups == 5 and p.parts == 11 and p.last == 5                        # several workgroups of pixels, the last one partly
    p = plans[(5, 256, 512, 13, 13, 1)]
    assert p.chunk == 9 and p.blocks == 64 and p.parts == 8 and p.last == 7 and p.straddle                 # more steps per part than the minimum
    assert plans[(2, 128, 256, 17, 17, 2)].blocks == 16 and plans[(1, 256, 512, 4, 5, 1)].blocks == 64
    assert any(not pl.odd_tail for pl in plans.values())


# ---------------------------------------------------------------- the torch route on the CPU
def test_conv4x4_train_on_the_cpu_is_conv2d():
    torch.manual_seed(0)
    for stride in (1, 2):
        x, w = torch.randn(2, 64, 9, 10, requires_grad=True), torch.randn(64, 64, 4, 4, requires_grad=True)
        y = DC.conv4x4_train(x, w, stride)
        want = F.conv2d(x, w, None, stride, 2)
        assert torch.equal(y, want) and "DiscConv" not in type(y.grad_fn).__name__
        g = torch.randn_like(y)
        for a, b in zip(torch.autograd.grad(y, (x, w), g), torch.autograd.grad(want, (x, w), g)):
            assert torch.equal(a, b)


def test_snconv_under_f16_on_the_cpu_is_conv2d():
    torch.manual_seed(1)
    opt = argparse.Namespace(isTrain=True)
    conv = _SNConv(64, 128, 4, 2, 2, opt).train()
    twin = _SNConv(64, 128, 4, 2, 2, opt).train()
    twin.load_state_dict(conv.state_dict())
    x = torch.randn(2, 64, 9, 9)
    with DC.discriminator_conv_train("f16"):
        y = conv(x)
    want = twin(x)
    assert torch.equal(y, want)
    g = torch.randn_like(y)
    y.backward(g)
    want.backward(g)
    assert torch.equal(conv.weight_orig.grad, twin.weight_orig.grad)


# ---------------------------------------------------------------- the stacked routes
def test_hip_routes_with_discriminator_forces_six_and_restores():
    assert len(training.HIP_ROUTES) == 5 and DC.discriminator_conv_train not in [s for s, _ in training.HIP_ROUTES]
    switches = [s for s, _ in training.HIP_ROUTES] + [DC.discriminator_conv_train]
    assert all(s.forced() is None for s in switches)
    with training.hip_routes_with_discriminator() as forced:
        assert len(forced) == 6 and forced["discriminator_conv_train"] == "f16"
        assert [s.forced() for s in switches] == [v for _, v in training.HIP_ROUTES] + ["f16"]
        with training.hip_routes() as inner:
            assert len(inner) == 5 and DC.discriminator_conv_train.forced() == "f16"
    assert all(s.forced() is None for s in switches)
    with training.hip_routes():
        assert DC.discriminator_conv_train.forced() is None


# ---------------------------------------------------------------- the reference's formulas
@pytest.mark.parametrize("shape", [(2, 3, 5, 1, 1, 1), (2, 3, 5, 1, 1, 2), (2, 3, 5, 5, 7, 2), (1, 4, 2, 6, 4, 2), (2, 3, 5, 9, 4, 1), (1, 2, 3, 2, 3, 2)],
                         ids=str)
def test_formulas_against_fp64_autograd(shape):
    B, Ci, Co, H, W, stride = shape
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, Ci, H, W, generator=gen, dtype=torch.double, requires_grad=True)
    w = torch.randn(Co, Ci, 4, 4, generator=gen, dtype=torch.double, requires_grad=True)
    y = F.conv2d(x, w, None, stride, 2)
    assert tuple(y.shape) == ref.out_shape(*shape)
    g = torch.randn(y.shape, generator=gen, dtype=torch.double)
    gx, gw = torch.autograd.grad(y, (x, w), g)
    assert (ref.grad_input(g, w.detach(), stride, H, W) - gx).abs().max() <= 1e-12
    assert (ref.grad_weight(x.detach(), g, stride) - gw).abs().max() <= 1e-12


def test_the_header_states_the_plan():
    text = open(os.path.join(abi_util.ROOT, "include", "pixelsynth_disc_conv.h")).read()
    for phrase in ("steps per part = max(8, ceil(steps / min(PS_DISC_CONV_MAX_PARTS, ceil(512 / blocks))))", "#define PS_DISC_CONV_MAX_PARTS 256",
                   "blocks         = (Co / 64) (Ci / 32)"):
        assert phrase in text, phrase


# ---------------------------------------------------------------- the tools
def test_the_tools_load_without_a_device(capsys):
    import importlib
    import sys
    tools = os.path.join(abi_util.ROOT, "tools")
    path = list(sys.path)
    try:
        sys.path.append(tools)
        timing, step = importlib.import_module("disc_conv_time"), importlib.import_module("train_step_time")
        with pytest.raises(SystemExit) as stop:
            timing.main(["--help"])
    finally:
        sys.path[:] = path
    assert stop.value.code == 0 and "usage:" in capsys.readouterr().out
    assert timing.SHAPES == [(64, 128, 129, 2), (128, 256, 65, 2), (256, 512, 33, 1), (64, 128, 65, 2), (128, 256, 33, 2), (256, 512, 17, 1)]
    assert list(step.ROUTES) == ["hip", "default", "hip+disc"] and step.ROUTES["hip+disc"] is training.hip_routes_with_discriminator
    # the new kernels' names fall into the step tool's class of convolutions
    assert all(any(s in k for s in step.CONV_NAMES) for k in timing.OURS)
