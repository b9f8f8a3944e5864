"""CPU-only: the host side of the depth Unet's training route (csrc/unet_train.hip, networks/unet_train.py): the registry entry and the C
ABI of libpixelsynth_unet_train.so against its header and bindings, the plan (a pure host function) against its mirrors, the refusals,
the switch and the training context, the routes on the host (all three are torch's expressions, bit for bit), and the fp64 mirrors, the
twin and the kink caps of tests/_unet_train_ref.py against torch's own operators and autograd."""
import copy
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _unet_train_ref as ref
from _forward_train_util import train_opts
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, training
from pixelsynth_amd.networks import architectures as arch, conv_routes, unet_train as UT

EPS = 1e-5


def test_the_registry_has_the_unet_train_library():
    names = [e.name for e in _libraries.LIBRARIES]
    at = names.index("unet_train")
    entry = _libraries.LIBRARIES[at]
    # in front of gan_train, which stays last -- and in front of disc_conv, which tests/test_disc_conv_cpu.py pins next to it
    assert names[-1] == "gan_train" and at == len(names) - 3 and names[at + 1] == "disc_conv" and list(_lib.PROTOS) == names
    assert entry.so == "libpixelsynth_unet_train.so" and entry.headers == ("pixelsynth_unet_train.h",)
    assert entry.last_error == "ps_unet_train_last_error"
    assert [u for u, _ in entry.units] == ["unet_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("unet_train")
    assert set(protos) == set(_lib.UNET_TRAIN_PROTOS) == {
        "ps_unet_train_last_error", "ps_unet_train_workspace_bytes", "ps_unet_train_parts", "ps_bn_stats_f32", "ps_bn_act_apply_f32",
        "ps_bn_act_backward_f32", "ps_relu_up2_cat_f32", "ps_relu_up2_cat_backward_f32"}
    assert _lib.PROTOS["unet_train"] is _lib.UNET_TRAIN_PROTOS
    header = open(os.path.join(ROOT, "include", "pixelsynth_unet_train.h")).read()
    for name, value, mine in (("MAX_PARTS", ref.MAX_PARTS, UT.MAX_PARTS), ("PART_ROWS", ref.PART_ROWS, UT.PART_ROWS), ("MAX_C", ref.MAX_C, UT.MAX_C)):
        assert int(re.search(r"#define PS_UNET_TRAIN_%s (\d+)" % name, header).group(1)) == value == mine
    # the pinned library does not export what this one adds; every call of the package goes through _lib.call
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)
    source = open(os.path.join(ROOT, "pixelsynth_amd", "networks", "unet_train.py")).read()
    assert set(re.findall(r"\"(ps_\w+)\"", source)) == set(protos) - {"ps_unet_train_last_error", "ps_unet_train_parts"}
    assert not re.search(r"_lib\.(library|lib)\(", source)


def test_the_plan_against_its_mirrors():
    L = _lib.library("unet_train")
    sizes = [(B * H * W, C) for B, H, W, C in ref.BN_SHAPES] + [(1, 4), (255, 8), (512, 1024), (2 ** 20, 64), (2 ** 31 - 1, 4), (3, 65536)]
    for N, C in sizes:
        assert L.ps_unet_train_parts(N, C) == ref.plan(N, C)[1] == UT.plan(N, C)[1], (N, C)
        assert L.ps_unet_train_workspace_bytes(N, C) == ref.workspace_bytes(N, C) == UT.workspace_bytes(N, C), (N, C)
        assert UT.plan(N, C) == ref.plan(N, C)
    # (rows per part, parts, channel quads, row lanes, chunks) at the edges BN_SHAPES stands on either side of
    assert ref.plan(256, 4) == (256, 1, 1, 256, 1) and ref.plan(257, 4) == (256, 2, 1, 256, 1)
    assert ref.plan(4, 256) == (256, 1, 64, 4, 1) and ref.plan(4, 260) == (256, 1, 64, 4, 2)
    assert ref.plan(65536, 4)[:2] == (256, 256) and ref.plan(65537, 4)[:2] == (512, 129)
    assert ref.plan(105, 12)[2:] == (3, 85, 1)                                   # 255 threads at work, one idle
    assert {(B * H * W, C) for B, H, W, C in ref.BN_SHAPES} >= {(256, 4), (257, 4), (4, 256), (4, 260), (65536, 4), (65537, 4), (105, 12)}
    for N, C in ((0, 4), (-1, 4), (4, 0), (4, 6), (4, 65540)):
        assert L.ps_unet_train_parts(N, C) == 0 and L.ps_unet_train_workspace_bytes(N, C) == 0
    # relu_up2_cat: one thread per float4 of the output, 256 to a workgroup -- the cases stand on both sides of one workgroup
    out4 = lambda s, c: s[0] * 4 * s[1] * s[2] * (c[0] + (c[1] or 0)) // 4
    assert out4((1, 8, 8), (4, None)) == 256 and out4((1, 8, 8), (4, 4)) == 512 and out4((1, 3, 11), (4, 4)) == 264
    assert (1, 8, 8) in ref.UP_SHAPES and (1, 3, 11) in ref.UP_SHAPES and {(4, None), (4, 4)} <= set(ref.UP_CHANNELS)


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("unet_train")
    err = L.ps_unet_train_last_error
    a = torch.zeros(64).data_ptr()
    big = 1 << 20
    assert L.ps_bn_stats_f32(None, 4, 4, EPS, 0.1, a, a, a, a, a, a, a, big, None) != 0 and b"bn_stats: null pointer" in err()
    assert L.ps_bn_stats_f32(a, 4, 6, EPS, 0.1, a, a, a, a, a, a, a, big, None) != 0 and b"C = 6 is not a multiple of 4" in err()
    assert L.ps_bn_stats_f32(a, 0, 4, EPS, 0.1, a, a, a, a, a, a, a, big, None) != 0 and b"expected both >= 1" in err()
    assert L.ps_bn_stats_f32(a, 4, 65540, EPS, 0.1, a, a, a, a, a, a, a, big, None) != 0 and b"more than 65536 channels" in err()
    assert L.ps_bn_stats_f32(a, 1, 4, EPS, 0.1, a, a, a, a, a, a, a, big, None) != 0 and b"the running variance needs N >= 2" in err()
    assert L.ps_bn_stats_f32(a, 4, 4, EPS, 0.1, a, None, a, a, a, a, a, big, None) != 0 and b"go together" in err()
    assert L.ps_bn_stats_f32(a + 4, 4, 4, EPS, 0.1, a, a, a, a, a, a, a, big, None) != 0 and b"aligned to 16 bytes" in err()
    assert L.ps_bn_stats_f32(a, 4, 4, EPS, 0.1, a, a, a, a, a, a, None, big, None) != 0 and b"null pointer (workspace)" in err()
    need = L.ps_unet_train_workspace_bytes(4, 4)
    assert L.ps_bn_stats_f32(a, 4, 4, EPS, 0.1, a, a, a, a, a, a, a, need - 1, None) != 0 and b"bytes, %d needed" % need in err()
    assert L.ps_bn_act_apply_f32(a, a, a, a, a, 4, 4, 0.2, None, a, None) != 0 and b"bn_act_apply: null pointer" in err()
    assert L.ps_bn_act_apply_f32(a, a, a, a, a, 4, 4, 0.2, a, a + 4, None) != 0 and b"aligned to 16 bytes" in err()
    assert L.ps_bn_act_backward_f32(a, None, None, a, a, a, a, 4, 4, 0.2, a, a, a, a, big, None) != 0 and b"(dy and dz)" in err()
    assert L.ps_bn_act_backward_f32(a, a, None, a, a, a, a, 4, 4, 0.2, a, None, a, a, big, None) != 0 and b"bn_act_backward: null pointer" in err()
    assert L.ps_relu_up2_cat_f32(a, None, 1, 2, 2, 4, 4, a, None) != 0 and b"b goes with Cb > 0" in err()
    assert L.ps_relu_up2_cat_f32(a, a, 1, 2, 2, 6, 4, a, None) != 0 and b"multiples of 4" in err()
    assert L.ps_relu_up2_cat_f32(a, a, 1, 0, 2, 4, 4, a, None) != 0 and b"expected all >= 1" in err()
    assert L.ps_relu_up2_cat_f32(a, a, 1, 2, 2, 4, 4, None, None) != 0 and b"relu_up2_cat: null pointer" in err()
    assert L.ps_relu_up2_cat_backward_f32(a, a, 1, 2, 2, 8, 4, 8, a, None) != 0 and b"c0 + Cs <= C" in err()
    assert L.ps_relu_up2_cat_backward_f32(a, a + 8, 1, 2, 2, 8, 4, 4, a, None) != 0 and b"aligned to 16 bytes" in err()
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match=r"ps_relu_up2_cat_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_relu_up2_cat_f32", z, None, 1, 1, 1, 4, 0, z)


def test_the_switch_and_the_training_context(monkeypatch):
    monkeypatch.setattr(UT, "UNET_TRAIN", UT.unet_train.from_env({}))
    assert UT.mode() == "torch" and UT.unet_train.default == "torch" and UT.unet_train.values == ("hip", "torch")
    assert UT.unet_train.env == "PS_UNET_TRAIN" and UT.unet_train.from_env({"PS_UNET_TRAIN": "hip"}) == "hip" and UT.unet_train.attr is None
    with UT.unet_train("hip"):
        assert UT.mode() == "hip"
        with UT.unet_train("torch"):
            assert UT.mode() == "torch"
        assert UT.mode() == "hip"
    assert UT.mode() == "torch"
    with pytest.raises(ValueError, match="'hip' or 'torch'"):
        UT.unet_train("triton")
    monkeypatch.setattr(UT, "UNET_TRAIN", "cuda")
    with pytest.raises(ValueError, match="'hip' or 'torch'"):
        UT.mode()
    assert len(training.HIP_ROUTES) == 5 and UT.unet_train not in [s for s, _ in training.HIP_ROUTES]
    with training.hip_routes_with_spectral() as inner:
        assert UT.unet_train.forced() is None
    with training.hip_routes_with_unet() as forced:
        assert forced == dict(inner, unet_train="hip") and UT.mode() == "hip"
    with training.hip_routes_with_spectral(discriminator=True) as inner:
        pass
    with training.hip_routes_with_unet(discriminator=True) as forced:
        assert forced == dict(inner, unet_train="hip") and forced["discriminator_conv_train"] == "f16"
    assert UT.unet_train.forced() is None
    # active(): the route, a CUDA fp32 input, grad mode or train() -- nothing on the host
    with UT.unet_train("hip"):
        assert not UT.active(nn.Identity().train(), torch.zeros(1, 3, 4, 4))


def test_takes_refuses_what_the_issue_names(monkeypatch):
    x = torch.randn(2, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    mod = nn.BatchNorm2d(8).train()
    assert not UT.takes_bn(x, mod) and not UT.takes_up(x) and not UT.takes_up(x, x)            # the CPU
    # the tensor's side: routing.gpu_f32 says no to each of these on any device
    for bad in (x.double(), x.contiguous(), torch.randn(2, 6, 3, 3).contiguous(memory_format=torch.channels_last), x.flatten()[1:].reshape(-1)):
        assert not UT.gpu_f32(bad, multiple=4, aligned=True)
    # the module's side, with the tensor's test out of the way
    monkeypatch.setattr(UT, "gpu_f32", lambda t, **k: t.dtype == torch.float32)
    assert UT.takes_bn(x, mod) and UT.takes_up(x) and UT.takes_up(x, x[:, :4])
    assert not UT.takes_bn(x[:1, :, :1, :1], mod)                                              # N = 1: torch raises
    assert UT.takes_bn(x[:1, :, :1, :2], mod)
    assert not UT.takes_bn(x, copy.deepcopy(mod).eval())
    assert not UT.takes_bn(x, nn.BatchNorm2d(8, momentum=None).train())
    assert not UT.takes_bn(x, nn.BatchNorm2d(8, track_running_stats=False).train())
    assert not UT.takes_bn(x, nn.BatchNorm2d(8, affine=False).train())
    assert not UT.takes_bn(x, nn.InstanceNorm2d(8, affine=True, track_running_stats=True).train())
    assert not UT.takes_bn(x, nn.SyncBatchNorm(8).train())
    assert not UT.takes_bn(x, copy.deepcopy(mod).double()) and not UT.takes_bn(x.double(), mod)
    assert not UT.takes_up(x, x[:1]) and not UT.takes_up(x, x[:, :, :2]) and not UT.takes_up(x, x.double())


def _unet(f=4, seed=0):
    torch.manual_seed(seed)
    return arch.Unet(num_filters=f, channels_in=3, channels_out=3, opt=train_opts()).train()


def test_on_the_host_every_route_is_torchs_bit_for_bit():
    x = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(1))
    runs = []
    for route in (None, "torch", "hip"):
        net = _unet()
        if route is None:
            y = net(x)
        else:
            with UT.unet_train(route):
                y = net(x)
        y.square().sum().backward()
        runs.append((y.detach(), [p.grad for p in net.parameters()], [b.clone() for b in net.buffers()]))
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0])
        assert all(torch.equal(s, t) for part in (1, 2) for s, t in zip(runs[0][part], other[part]))
    # the two functions alone, and the conv route: nothing on the host
    mod, h = nn.BatchNorm2d(8).train(), torch.randn(2, 8, 5, 5)
    twin = copy.deepcopy(mod)
    with UT.unet_train("hip"):
        y, z = UT.bn_act_train(h, mod, 0.2)
        up = UT.relu_up2_cat(h, h[:, :4])
        assert conv_routes._unet_train_conv(nn.Conv2d(64, 64, 3, padding=1), torch.randn(1, 64, 16, 16)) is None
    assert torch.equal(y, twin(h)) and torch.equal(z, F.leaky_relu(y, 0.2)) and torch.equal(mod.running_var, twin.running_var)
    assert torch.equal(up, F.interpolate(F.relu(torch.cat((h, h[:, :4]), 1)), scale_factor=2, mode="bilinear", align_corners=False))
    assert torch.equal(UT.bn_act_train(h, mod), twin(h))


def test_the_twin_is_unet_forward():
    net, x = _unet(seed=3), torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(2))
    a, b, c = copy.deepcopy(net), copy.deepcopy(net), copy.deepcopy(net)
    want = net(x)
    assert torch.equal(ref.twin_forward(a, x), want)
    # its own decisions, recorded and replayed: the same values, nothing differs
    seen = ref.Decisions()
    h = x
    real = (F.leaky_relu, F.relu)
    try:
        F.leaky_relu = lambda t, s: (seen.record(t), real[0](t, s))[1]
        F.relu = lambda t: (seen.record(t), real[1](t))[1]
        ref.twin_forward(c, h)
    finally:
        F.leaky_relu, F.relu = real
    assert len(seen.masks) == 15
    got = ref.twin_forward(b, x, seen)
    assert seen.differ == 0 and seen.total > 0 and (got - want).abs().max() <= 1e-6 * want.abs().max()


@pytest.mark.parametrize("shape", ref.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_batch_norm_mirror_is_torchs(shape):
    B, H, W, C = shape
    x, weight, bias, dy, dz = ref.bn_inputs(B, H, W, C, seed=B + H + W + C)
    f = ref.bn_forward64(x, weight, bias, EPS, ref.SLOPE)
    y64 = F.batch_norm(x.double(), None, None, weight.double(), bias.double(), True, 0.1, EPS)
    assert (f["y"] - y64).abs().max() <= 1e-12 * (1 + y64.abs().max())
    assert torch.equal(f["z"], torch.where(f["y"] > 0, f["y"], 0.2 * f["y"]))
    # no decision of the leaky ReLU is in doubt in fp32, and the fp64 reference alone stays inside the kink cap
    assert (f["y"].abs() > ref.forward_bound(x, f)).all() and ref.kink_free(f["y"])[1] <= ref.KINK_SHARE
    for gy, gz in ((dy, None), (None, dz), (dy, dz)):
        want = ref.bn_backward64(x, gy, gz, weight, bias, EPS, ref.SLOPE)
        auto = ref.bn_autograd(x, weight, bias, gy, gz, EPS, ref.SLOPE, torch.float64)
        for a, b in zip(want, auto):
            assert (a - b).abs().max() <= 1e-10 * (1 + b.abs().max())
    # torch's fp32 y is inside the bound; a value off by one part in 10^5 is not
    y32 = F.batch_norm(x, None, None, weight, bias, True, 0.1, EPS)
    bound = ref.forward_bound(x, f)
    assert ref.check(f"{shape} torch fp32 y", y32, f["y"], bound) <= 1.0
    assert ref.check(f"{shape} y off", f["y"].float() * (1 + 1e-5) + 1e-5, f["y"], bound) > 1.0


def test_the_running_mirror_is_torchs():
    x1, weight, bias, _, _ = ref.bn_inputs(3, 5, 7, 12, seed=11)
    x2 = ref.bn_inputs(3, 5, 7, 12, seed=12, offset=-0.7, spread=0.5)[0]
    mod = nn.BatchNorm2d(12).double().train()
    m32 = nn.BatchNorm2d(12).train()
    for calls, x in enumerate((x1, x2), 1):
        rm, rv, rm32, rv32 = mod.running_mean.clone(), mod.running_var.clone(), m32.running_mean.clone(), m32.running_var.clone()
        mod(x.double()), m32(x)
        rm64, rv64, bm, bv = ref.running64(rm, rv, x, 0.1)
        assert (mod.running_mean - rm64).abs().max() <= 1e-14 and (mod.running_var - rv64).abs().max() <= 1e-14
        assert int(mod.num_batches_tracked) == calls and (bm > 0).all() and (bv > 0).all()
        # a wrong formula is outside: the biased variance stored, or the momentum on the wrong side
        rm64, rv64, bm, bv = ref.running64(rm32, rv32, x, 0.1)
        var = ref.stats64(x)[1]
        assert ((rv32.double() * 0.9 + 0.1 * var - rv64).abs() > bv).all()
        assert ((rm32.double() * 0.1 + 0.9 * ref.stats64(x)[0] - rm64).abs() > bm).any()


@pytest.mark.parametrize("shape", ref.UP_SHAPES + [ref.UP_WIDE[0]], ids=lambda s: "x".join(map(str, s)))
def test_the_upsampling_mirror_is_torchs(shape):
    B, H, W = shape
    for Ca, Cb in (ref.UP_CHANNELS if shape != ref.UP_WIDE[0] else [ref.UP_WIDE[1]]):
        gen = torch.Generator().manual_seed(H * 100 + W * 10 + Ca)
        a = torch.randn(B, Ca, H, W, generator=gen)
        b = None if Cb is None else torch.randn(B, Cb, H, W, generator=gen)
        g = torch.randn(B, Ca + (Cb or 0), 2 * H, 2 * W, generator=gen)
        out, mag = ref.up_forward64(a, b)
        want = F.interpolate(F.relu(ref.up_cat(a, b).double()), scale_factor=2, mode="bilinear", align_corners=False)
        assert (out - want).abs().max() <= 1e-14 * (1 + want.abs().max())
        auto = ref.up_autograd(a, b, g, torch.float64)
        c0 = 0
        for src, d in zip((a, b), auto):
            if src is None:
                continue
            grad, mag, k = ref.up_adjoint64(g, src, c0)
            c0 += src.size(1)
            assert (grad - d).abs().max() <= 1e-13 * (1 + d.abs().max()) and 4 <= int(k.max()) <= 16
            assert ref.kink_free(src)[1] <= ref.KINK_SHARE                     # the reference alone stays inside the cap
    My = ref.up_matrix(5)
    assert torch.equal(My.sum(1), torch.ones(10, dtype=torch.float64)) and My[0, 0] == 1 and My[9, 4] == 1 and My[1, 0] == 0.75 and My[2, 1] == 0.75
    assert torch.equal(ref.up_matrix(1), torch.ones(2, 1, dtype=torch.float64))


def test_the_tools_load_without_a_device(capsys):
    import importlib
    import sys
    path = list(sys.path)
    try:
        sys.path.append(os.path.join(ROOT, "tools"))
        timing, step = importlib.import_module("unet_train_time"), importlib.import_module("train_step_time")
        with pytest.raises(SystemExit) as stop:
            timing.main(["--help"])
    finally:
        sys.path[:] = path
    assert stop.value.code == 0 and "--layers" in capsys.readouterr().out
    assert step.UNET_ROUTES == {"hip+sn+unet": training.hip_routes_with_unet} and "hip+sn+unet" not in step.ROUTES
    # every kernel of the unit has a name the tool files under "new kernels", and none of them under another class
    source = open(os.path.join(ROOT, "pixelsynth_amd", "csrc", "unet_train.hip")).read()
    kernels = re.findall(r"__global__ [^\n]*void (k_\w+)\(", source)
    assert sorted(kernels) == sorted(timing.OURS) and len(kernels) == 8
    assert all(timing.class_of(f"void (anonymous namespace)::{k}(float const*)") == "new kernels" for k in kernels)
    assert timing.class_of("k_conv3x3_f16x3<4>") == "3 x 3 products" and timing.class_of("k_thin_expand") == "3 x 3 products"
    assert timing.class_of("miopen_wrw_gemm") == "library convolutions" and timing.class_of("vectorized_elementwise_kernel") == "everything else"
