"""CPU: the training step's glue (networks/train_glue.py, csrc/train_glue.hip behind include/pixelsynth_train_glue.h) as far as it goes
without a GPU: the library, its header and its prototype table agree and its entry points refuse bad arguments before a launch; the
torch route of combine_mask_nhwc is get_combined + the decoder's concatenation on the reference's recorded blend; both Functions' torch
routes under gradcheck; the depth head's fp64 formula and torch's fp32 one within the derived bound on the host; the switch's order of
precedence; what "hip" declines."""
import os
import re
import types

import numpy as np
import pytest
import torch

import _train_glue_ref as ref
from abi_util import assert_library_matches_header
from pixelsynth_amd import _lib, training
from pixelsynth_amd.networks import train_glue as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_library_header_and_prototypes_agree():
    protos = assert_library_matches_header("train_glue")
    assert len(protos) == 5
    hdr = open(os.path.join(ROOT, "include", "pixelsynth_train_glue.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (PS_GLUE_\w+) (\d+)", hdr)}
    assert (defs["PS_GLUE_DEPTH_RANGE"], defs["PS_GLUE_DEPTH_INVERSE"]) == (tg.DEPTH_RANGE, tg.DEPTH_INVERSE) == (ref.RANGE, ref.INVERSE)


def test_entry_points_refuse_bad_arguments_before_a_launch():
    L = _lib.library("train_glue")
    one = torch.zeros(16)
    p, err = one.data_ptr(), L.ps_train_glue_last_error
    assert L.ps_combine_mask_nhwc_f32(None, p, p, 1, 1, 1, p, None) < 0 and b"null" in err()
    assert L.ps_combine_mask_nhwc_f32(p, p, p, 0, 1, 1, p, None) < 0 and b"B = 0" in err()
    assert L.ps_combine_mask_nhwc_f32(p, p, p, 65536, 256, 256, p, None) < 0 and b"2^31" in err()
    assert L.ps_combine_mask_nhwc_f32(p, p, p, 1, 1, 1, p + 4, None) < 0 and b"16 bytes" in err()
    assert L.ps_combine_mask_nhwc_backward_f32(p, None, 1, 1, 1, p, None) < 0 and b"null" in err()
    assert L.ps_combine_mask_nhwc_backward_f32(p + 4, p, 1, 1, 1, p, None) < 0 and b"16 bytes" in err()
    assert L.ps_depth_head_forward_f32(p, 2, 0.5, 10.0, 1, p, p, None) < 0 and b"mode = 2" in err()
    assert L.ps_depth_head_forward_f32(p, 0, 0.5, 10.0, 0, p, p, None) < 0 and b"N = 0" in err()
    assert L.ps_depth_head_forward_f32(p, 0, 0.5, 10.0, 2 ** 31, p, p, None) < 0 and b"2^31" in err()
    assert L.ps_depth_head_forward_f32(p, 0, float("nan"), 10.0, 1, p, p, None) < 0 and b"finite" in err()
    assert L.ps_depth_head_forward_f32(p, 0, 0.5, 10.0, 1, p, None, None) < 0 and b"null" in err()
    assert L.ps_depth_head_backward_f32(p, p, 0, 0.5, 10.0, 1, None, None) < 0 and b"null" in err()
    assert L.ps_depth_head_backward_f32(p, p, -1, 0.5, 10.0, 1, p, None) < 0 and b"mode = -1" in err()
    with pytest.raises(RuntimeError, match=r"ps_depth_head_forward_f32: args\[0\] is a CPU tensor"):
        _lib.call("ps_depth_head_forward_f32", one, 0, 0.5, 10.0, 16, one, one)


def test_torch_route_is_get_combined_and_the_mask_channel_on_the_recorded_blend():
    """comb_* of poses.npz: inputs and the output of the REFERENCE's get_combined"""
    fx = np.load(os.path.join(GOLD, "poses.npz"))
    gen, ar, bg = (torch.from_numpy(fx[k]) for k in ("comb_gen", "comb_ar", "comb_bg"))
    with tg.train_glue("torch"):
        out = tg.combine_mask_nhwc(gen, ar, bg)
    assert out.shape == (gen.size(0), gen.size(1) + 1, gen.size(2), gen.size(3))
    np.testing.assert_array_equal(out[:, :-1].numpy(), fx["comb_out"])
    np.testing.assert_array_equal(out[:, -1].numpy(), (~bg).float().numpy())
    # the default route ("hip") declines CPU tensors and gives the same
    assert torch.equal(tg.combine_mask_nhwc(gen, ar, bg), out)
    assert ref.same_bits(out, ref.combine_formula(gen, ar, bg))


def test_torch_routes_gradcheck():
    gen = torch.Generator().manual_seed(0)
    g = torch.randn(2, 3, 4, 5, dtype=torch.float64, generator=gen).requires_grad_()
    t = torch.randn(2, 3, 4, 5, dtype=torch.float64, generator=gen).requires_grad_()
    m = torch.rand(2, 4, 5, generator=gen) > 0.5
    assert m.any() and not m.all()
    assert torch.autograd.gradcheck(lambda a, b: tg.combine_mask_nhwc(a, b, m), (g, t))
    raw = ref.raws((2, 1, 4, 5), "randn").double().requires_grad_()
    for mode in (tg.DEPTH_RANGE, tg.DEPTH_INVERSE):
        assert torch.autograd.gradcheck(lambda a: tg.depth_head(a, mode, ref.MIN_Z, ref.MAX_Z)[0], (raw,))
        depth, pred = tg.depth_head(raw, mode, ref.MIN_Z, ref.MAX_Z)
        assert not pred.requires_grad and torch.equal(pred, depth.detach() / 5 - 1)
        assert torch.equal(depth, ref.depth_formula(raw, mode))
    with pytest.raises(ValueError, match="mode is 2"):
        tg.depth_head(raw, 2, 0.5, 10.0)


@pytest.mark.parametrize("mode", [ref.RANGE, ref.INVERSE])
@pytest.mark.parametrize("kind", ["randn", "large"])
def test_depth_bound_holds_for_torchs_own_fp32_on_the_host(mode, kind):
    """The derived bound is not so tight that a correctly rounded fp32 evaluation misses it, and not empty: torch's own fp32 formula"""
    raw = ref.raws((2, 1, 16, 16), kind)
    d64, bound = ref.depth_bound(raw, mode)
    assert ref.check(f"host fp32 depth mode {mode} {kind}", ref.depth_formula(raw, mode), d64, bound) <= 1.0
    assert (bound > 0).all() and (bound <= 16 * ref.U * d64.abs().clamp_min(ref.MIN_Z if mode == ref.RANGE else 0.0) + 1e-300).all()


def test_switch(monkeypatch):
    sw = tg.train_glue
    assert sw.default == "hip" and sw.env == "PS_TRAIN_GLUE" and sw.attr == "train_glue" and sw.values == ("hip", "torch")
    assert sw.from_env({}) == "hip" and sw.from_env({"PS_TRAIN_GLUE": "torch"}) == "torch"
    monkeypatch.setattr(tg, "TRAIN_GLUE", "hip")
    opt_none, opt_torch = types.SimpleNamespace(), types.SimpleNamespace(train_glue="torch")
    assert tg.mode() == tg.mode(opt_none) == "hip" and tg.mode(opt_torch) == "torch"         # the option over the process default
    monkeypatch.setattr(tg, "TRAIN_GLUE", "torch")
    assert tg.mode() == "torch" and tg.mode(types.SimpleNamespace(train_glue="hip")) == "hip"
    with sw("hip"):                                                                           # the block over the option
        assert tg.mode(opt_torch) == "hip" and sw.forced() == "hip"
        with sw("torch"):
            assert tg.mode(types.SimpleNamespace(train_glue="hip")) == "torch"
    assert sw.forced() is None
    with pytest.raises(ValueError, match="train_glue"):
        sw("HIP")
    monkeypatch.setattr(tg, "TRAIN_GLUE", "HIP")
    with pytest.raises(ValueError, match="PS_TRAIN_GLUE = 'HIP'"):
        tg.mode()


def test_hip_routes_forces_every_training_switch_and_restores_it():
    names = [s.name for s, _ in training.HIP_ROUTES]
    assert names == ["decoder_conv_train", "decoder_block_train", "decoder_thin_train", "pixelcnn_train", "train_glue"]
    before = [s.forced() for s, _ in training.HIP_ROUTES]
    with tg.train_glue("torch"):
        with training.hip_routes() as modes:
            assert modes == dict(zip(names, ["f16x3", "hip", "hip", "hip", "hip"]))
            assert all(s.resolve(types.SimpleNamespace(**{s.attr: "torch"}) if s.attr else None) == v for s, v in training.HIP_ROUTES)
        assert tg.mode() == "torch"
    assert [s.forced() for s, _ in training.HIP_ROUTES] == before


def test_hip_declines_what_the_kernels_do_not_take():
    g, t, m = torch.randn(2, 3, 4, 5), torch.randn(2, 3, 4, 5), torch.rand(2, 4, 5) > 0.5
    assert not tg.combine_takes(g, t, m) and not tg.depth_takes(torch.randn(2, 1, 4, 5))          # the CPU
    with tg.train_glue("hip"):                      # ... and the front ends go through the formula: no library call on a CPU tensor
        assert ref.same_bits(tg.combine_mask_nhwc(g, t, m), ref.combine_formula(g, t, m))
        d, p = tg.depth_head(torch.randn(2, 1, 4, 5), 0, 0.5, 10.0)
        assert d.shape == p.shape == (2, 1, 4, 5)
    # what would be declined on the device as well, seen through meta tensors' properties: the tests of takes() on shapes and types
    fake = lambda *shape, dtype=torch.float32: types.SimpleNamespace(
        is_cuda=True, dtype=dtype, shape=torch.Size(shape), device="cuda:0", requires_grad=False, dim=lambda: len(shape),
        size=lambda i=None: torch.Size(shape) if i is None else shape[i], numel=lambda: int(np.prod(shape)),
        is_contiguous=lambda memory_format=None: True)
    assert tg.depth_takes(fake(2, 1, 4, 5))
    assert not tg.depth_takes(fake(2, 2, 4, 5)) and not tg.depth_takes(fake(2, 1, 4, 5, dtype=torch.float64)) and not tg.depth_takes(fake(2, 1, 4))


def test_forward_train_needs_a_loss_and_a_target():
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts
    o = dict(W=256, use_rgb_features=True, splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=128, tau=1.0,
             rad_pow=2, accumulation="alphacomposite", background_smoothing_kernel_size=13, min_z=1.0, max_z=100.0,
             rotation=0.6, direction="R", temperature=0.7, model_setting="train", seed=0, homography=False)
    m = ZbufferModelPts(types.SimpleNamespace(**o))
    assert not hasattr(m, "loss_function")
    img, cam = torch.zeros(1, 3, 256, 256), {k: torch.eye(4)[None] for k in ("K", "Kinv", "P", "Pinv")}
    with pytest.raises(ValueError, match="carries the target view"):
        m(dict(images=[img], cameras=[cam]))
    with pytest.raises(RuntimeError, match="no loss_function"):
        m(dict(images=[img, img], cameras=[cam, cam]))
