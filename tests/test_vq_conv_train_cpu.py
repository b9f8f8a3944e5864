"""CPU-only: the host side of the VQ-VAE's training convolutions (csrc/vq_conv_train.hip, vqvae2/conv_train.py): the registry entry and
the C ABI of libpixelsynth_vq_conv_train.so against its header and bindings, the split into parts against its mirror, the mirrors of the
folds, the two adjoint identities the Functions rest on and the ends' correlation formula against torch's fp64 operators and autograd,
the refusals, and the switch."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _vq_conv_train_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries
from pixelsynth_amd import vqvae2
from pixelsynth_amd.vqvae2 import conv_train as CT, train as vq_train, vqvae as V

D = torch.double


def test_the_registry_has_the_vq_conv_train_library():
    names = [e.name for e in _libraries.LIBRARIES]
    at = names.index("vq_conv_train")
    entry = _libraries.LIBRARIES[at]
    assert names[at + 1:] == ["unet_train", "disc_conv", "gan_train"] and list(_lib.PROTOS) == names       # in front of unet_train
    assert entry.so == "libpixelsynth_vq_conv_train.so" and entry.headers == ("pixelsynth_vq_conv_train.h",)
    assert entry.last_error == "ps_vq_conv_train_last_error"
    assert [u for u, _ in entry.units] == ["vq_conv_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("vq_conv_train")
    assert set(protos) == set(_lib.VQ_CONV_TRAIN_PROTOS) == {
        "ps_vq_conv_train_last_error", "ps_vq_conv_train_parts", "ps_vq_conv_train_workspace_bytes", "ps_vq_relu_pack_f32", "ps_vq_gate_f32",
        "ps_vq_fold_f32", "ps_vq_ends_grad_weight_f32", "ps_vq_head_grad_input_f32"}
    assert _lib.PROTOS["vq_conv_train"] is _lib.VQ_CONV_TRAIN_PROTOS
    header = open(os.path.join(ROOT, "include", "pixelsynth_vq_conv_train.h")).read()
    for name, value in (("MAX_PARTS", ref.MAX_PARTS), ("MIN_PART", ref.MIN_PART), ("GROUPS", ref.GROUPS)):
        assert int(re.search(r"#define PS_VQ_CONV_TRAIN_%s (\d+)" % name, header).group(1)) == value
    # the pinned library does not export what this one adds; every call of the package goes through _lib.call
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)
    source = open(os.path.join(ROOT, "pixelsynth_amd", "vqvae2", "conv_train.py")).read()
    mine = {fn for fn in re.findall(r"\"(ps_\w+)\"", source) if fn in protos}
    assert mine == set(protos) - {"ps_vq_conv_train_last_error", "ps_vq_conv_train_parts"}
    assert not re.search(r"_lib\.(library|lib)\(", source)


def test_the_split_into_parts_against_its_mirror():
    L = _lib.library("vq_conv_train")
    for P in (1, 15, 16, 17, 255, 256, 257, 512, 513, 4096, 4097, 65536, 65537, 256 * 256 * 16, 256 * 256 * 16 + 1, 64 * 128 * 128,
              2 ** 31 - 1):
        rs = ref.part_ranges(P)
        assert L.ps_vq_conv_train_parts(P) == len(rs) <= ref.MAX_PARTS, P
        assert L.ps_vq_conv_train_workspace_bytes(P) == ref.workspace_bytes(P), P
        assert rs[0][0] == 0 and rs[-1][1] == P and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
        assert all((hi - lo) % ref.GROUPS == 0 and hi - lo >= ref.MIN_PART for lo, hi in rs[:-1])
    assert len(ref.part_ranges(64 * 128 * 128)) == 256 and ref.chain(64 * 128 * 128) == 256 + 16
    for P in (0, -1, 2 ** 31, 2 ** 40):
        assert L.ps_vq_conv_train_parts(P) == 0 and L.ps_vq_conv_train_workspace_bytes(P) == 0


def test_the_entry_points_refuse_before_they_launch():
    L = _lib.library("vq_conv_train")
    err = L.ps_vq_conv_train_last_error
    assert L.ps_vq_relu_pack_f32(None, 1, 2, 2, 4, 1, 0, None, None) != 0 and b"null" in err()
    assert L.ps_vq_relu_pack_f32(16, 1, 2, 2, 6, 1, 0, 32, None) != 0 and b"multiple of 4" in err()
    assert L.ps_vq_relu_pack_f32(16, 1, 3, 2, 4, 1, 1, 32, None) != 0 and b"even" in err()
    assert L.ps_vq_gate_f32(16, None, None, None, 6, None) != 0 and b"multiple of 4" in err()
    assert L.ps_vq_gate_f32(16, 16, None, None, 8, None) != 0 and b"gx is x" in err()
    assert L.ps_vq_fold_f32(16, 0, 64, 0, 32, None) != 0
    assert L.ps_vq_ends_grad_weight_f32(16, 32, 1, 6, 8, 1, 48, None, 64, 1 << 20, None) != 0 and b"multiples of 4" in err()
    assert L.ps_vq_ends_grad_weight_f32(16, 32, 1, 8, 8, 1, 48, None, 64, 16, None) != 0 and b"workspace" in err()
    assert L.ps_vq_head_grad_input_f32(16, 32, 48, 1, 4, 8, 64, None) != 0 and b"multiple of 16" in err()


def test_the_folds_invert_the_block_weights_on_their_live_positions():
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(5, 3, 4, 4, generator=gen)
    w3 = V.s2d_weight(w)
    assert torch.equal(ref.fold(w3), w)
    wt = torch.randn(3, 5, 4, 4, generator=gen)
    w3t = V.convt_weight(wt)
    assert torch.equal(ref.fold_t(w3t), wt)
    # the other 20 of the 36 (block, sub-position) pairs are zero: folding back and spreading again gives the same tensor
    for full, back in ((w3, V.s2d_weight(ref.fold(w3))), (w3t, V.convt_weight(ref.fold_t(w3t)))):
        assert torch.equal(full, back)
    live = V.s2d_weight(torch.ones(1, 1, 4, 4)).reshape(2, 2, 3, 3)
    assert int(live.sum()) == 16 and int((live == 0).sum()) == 20
    live = V.convt_weight(torch.ones(1, 1, 4, 4)).reshape(2, 2, 3, 3)
    assert int(live.sum()) == 16 and int((live == 0).sum()) == 20
    # the kernel's operand layouts
    assert torch.equal(ref.fold_kernel_layout(w3.permute(0, 2, 3, 1).contiguous(), False), w)
    assert torch.equal(ref.fold_kernel_layout(w3t.permute(0, 2, 3, 1).contiguous(), True), wt)


def test_the_two_adjoint_identities_in_fp64():
    gen = torch.Generator().manual_seed(5)
    B, Ci, Co, H, W = 2, 3, 5, 8, 12
    # the stride-2 convolution: forward = 3 x 3 over blocks; input gradient = d2s of the 3 x 3 convolution with convt_weight of the same tensor
    x = torch.randn(B, Ci, H, W, dtype=D, generator=gen, requires_grad=True)
    w = torch.randn(Co, Ci, 4, 4, dtype=D, generator=gen, requires_grad=True)
    g = torch.randn(B, Co, H // 2, W // 2, dtype=D, generator=gen)
    y = F.conv2d(x, w, None, 2, 1)
    assert torch.allclose(y, F.conv2d(V._s2d(x), V.s2d_weight(w), None, 1, 1), rtol=0, atol=1e-12)
    gx, gw = torch.autograd.grad(y, (x, w), g)
    mine = V._d2s(F.conv2d(g, V.convt_weight(w.detach()), None, 1, 1), Ci)
    assert torch.allclose(mine, gx, rtol=0, atol=1e-12)
    assert torch.allclose(mine, F.conv_transpose2d(g, w.detach(), None, 2, 1), rtol=0, atol=1e-12)
    import _conv_bwd_ref as cref
    assert torch.allclose(ref.fold(cref.wgrad(V._s2d(x.detach()).contiguous(), g)), gw, rtol=0, atol=1e-11)
    # the transposed convolution: forward = d2s of the 3 x 3 with convt_weight; input gradient = the stride-2 convolution of the same tensor
    x = torch.randn(B, Ci, H // 2, W // 2, dtype=D, generator=gen, requires_grad=True)
    wt = torch.randn(Ci, Co, 4, 4, dtype=D, generator=gen, requires_grad=True)
    g = torch.randn(B, Co, H, W, dtype=D, generator=gen)
    y = F.conv_transpose2d(x, wt, None, 2, 1)
    assert torch.allclose(y, V._d2s(F.conv2d(x, V.convt_weight(wt), None, 1, 1), Co), rtol=0, atol=1e-12)
    gx, gw = torch.autograd.grad(y, (x, wt), g)
    mine = F.conv2d(V._s2d(g), V.s2d_weight(wt.detach()), None, 1, 1)
    assert torch.allclose(mine, gx, rtol=0, atol=1e-12)
    assert torch.allclose(mine, F.conv2d(g, wt.detach(), None, 2, 1), rtol=0, atol=1e-12)
    assert torch.allclose(ref.fold_t(cref.wgrad(x.detach(), V._s2d(g).contiguous())), gw, rtol=0, atol=1e-11)


def test_the_ends_correlation_formula_against_fp64_autograd():
    gen = torch.Generator().manual_seed(7)
    B, H, W = 2, 8, 16
    img = torch.randn(B, 3, H, W, dtype=D, generator=gen)
    # the stem
    w = torch.randn(64, 3, 4, 4, dtype=D, generator=gen, requires_grad=True)
    b = torch.randn(64, dtype=D, generator=gen, requires_grad=True)
    g = torch.randn(B, 64, H // 2, W // 2, dtype=D, generator=gen)
    gw, gb = torch.autograd.grad(F.conv2d(img, w, b, 2, 1), (w, b), g)
    assert torch.allclose(ref.ends_dw(img, g), gw, rtol=0, atol=1e-11) and torch.allclose(g.sum((0, 2, 3)), gb, rtol=0, atol=1e-11)
    # the head: wide = relu(h), img = the image's gradient
    h = torch.randn(B, 64, H // 2, W // 2, dtype=D, generator=gen, requires_grad=True)
    wt = torch.randn(64, 3, 4, 4, dtype=D, generator=gen, requires_grad=True)
    bt = torch.randn(3, dtype=D, generator=gen, requires_grad=True)
    gi = torch.randn(B, 3, H, W, dtype=D, generator=gen)
    gh, gw, gb = torch.autograd.grad(F.conv_transpose2d(F.relu(h), wt, bt, 2, 1), (h, wt, bt), gi)
    assert torch.allclose(ref.ends_dw(gi, F.relu(h.detach())), gw, rtol=0, atol=1e-11)
    assert torch.allclose(gi.sum((0, 2, 3)), gb, rtol=0, atol=1e-11)
    assert torch.allclose(ref.head_gin(gi, wt.detach()) * (h.detach() > 0), gh, rtol=0, atol=1e-11)
    # the blocked form the stem's gradient arrives in
    blocked = V._s2d(g).permute(0, 2, 3, 1)
    y, x, o = 3, 5, 17
    assert blocked[1, y // 2, x // 2, ((y & 1) * 2 + (x & 1)) * 64 + o] == g[1, o, y, x]


def test_the_functions_refuse_what_they_do_not_take():
    x = torch.randn(1, 64, 16, 16).contiguous(memory_format=torch.channels_last)
    w3, w4, b = torch.randn(64, 64, 3, 3), torch.randn(64, 64, 4, 4), torch.randn(64)
    calls = [lambda: CT.conv3x3_relu_train(x, w3, b, True), lambda: CT.conv4x4s2_train(x, w4, b, True),
             lambda: CT.convt4x4s2_train(x, w4, b, True), lambda: CT.conv1x1_relu_train(x, torch.randn(64, 64, 1, 1), b),
             lambda: CT.res_block_train(x, torch.randn(32, 64, 3, 3), torch.randn(32), torch.randn(64, 32, 1, 1), b),
             lambda: CT.stem_train(torch.randn(1, 3, 16, 16), torch.randn(64, 3, 4, 4), b),
             lambda: CT.head_train(x, torch.randn(64, 3, 4, 4), torch.randn(3))]
    for call in calls:            # the CPU
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        CT.conv3x3_relu_train(x.double(), w3.double(), b.double(), True)


def test_the_switch(monkeypatch):
    monkeypatch.setattr(V, "VQVAE_TRAIN", V.vqvae_train.from_env({}))
    sw = vqvae2.vqvae_train
    assert sw is V.vqvae_train and sw.resolve() == "torch" and sw.default == "torch" and sw.values == ("hip", "torch")
    assert sw.env == "PS_VQVAE_TRAIN" and sw.from_env({"PS_VQVAE_TRAIN": "hip"}) == "hip" and sw.attr is None
    with sw("hip"):
        assert sw.resolve() == "hip"
        with sw("torch"):
            assert sw.resolve() == "torch"
    with pytest.raises(ValueError):
        sw("triton")
    monkeypatch.setattr(V, "VQVAE_TRAIN", "hipp")          # a misspelt PS_VQVAE_TRAIN
    with pytest.raises(ValueError, match="PS_VQVAE_TRAIN"):
        V.VQVAETop().eval()(torch.zeros(1, 3, 128, 128))
    with pytest.raises(ValueError, match="PS_VQVAE_TRAIN"):
        vq_train.train_step(V.VQVAETop(), None, torch.zeros(1, 3, 128, 128))


def _graph_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo += [f for f, _ in fn.next_functions]
    return names


def test_no_function_in_the_graph_under_torch_or_on_the_cpu(monkeypatch):
    monkeypatch.setattr(V, "VQVAE_TRAIN", "torch")

    def nearest(self, z, layout, hw=1):          # (the quantiser's kernel has no CPU route; the convolutions are what this test is about)
        assert layout == 0
        return (z.pow(2).sum(1, keepdim=True) - 2 * z @ self.embed + self.embed.pow(2).sum(0)).argmin(1).to(torch.int32)
    monkeypatch.setattr(V.Quantize, "nearest", nearest)
    torch.manual_seed(0)
    m = V.VQVAETop().eval()          # (eval: the quantiser's training half has no CPU route; the convolutions are the same expressions)
    x = torch.rand(1, 3, 128, 128)
    mine = ("_ConvForm", "_ResBlock", "_Conv1x1Relu", "_Stem", "_Head", "_Conv1x1Train")
    outs = []
    for route in ("torch", "hip"):
        with V.vqvae_train(route):
            out, diff = m(x)
        names = _graph_names(out) | _graph_names(diff)
        assert not any(n.startswith(mine) for n in names), (route, names)
        outs.append((out, diff))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not CT.takes(m, x) and not CT.takes(m, x.double())
