"""CPU: the training step (base_model.BaseModel) against the REFERENCE's own BaseModel.__call__ (tests/golden/train_forward.npz, part
(b): two calls in a row on a one-convolution stand-in generator at 32 x 32 with ndf = 8, with and without normalize_image): the merged
loss dicts -- keys exactly, values rtol 1e-5 -- and every recorded parameter value after each call, rtol 1e-4, as
tests/test_gan_train_cpu.py holds the discriminator's step to gan_train.npz; what BaseModel builds and refuses; and forward_train's
host logic (dispatch, loss assembly, output keys) on the CPU with the renderer replaced by a stand-in and outpainting off.

Part (a) of the fixture, the reference's forward in 'train', is compared in tests/test_forward_train_gpu.py: this project's nearest-code
search, plan masks and masked convolution exist on the device alone, so its forward with outpainting does not run on the CPU."""
import os

import numpy as np
import pytest
import torch

import _forward_train_util as U
from pixelsynth_amd import compat
from pixelsynth_amd.base_model import BaseModel
from pixelsynth_amd.losses.gan_loss import DiscriminatorLoss

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_forward.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


def test_fixture_stays_below_the_largest_golden_file():
    sizes = {f: os.path.getsize(os.path.join(os.path.dirname(GOLD), f)) for f in os.listdir(os.path.dirname(GOLD)) if f.endswith(".npz")}
    assert sizes["train_forward.npz"] < max(v for k, v in sizes.items() if k != "train_forward.npz")


@pytest.mark.parametrize("tag,normalize", [("step_plain", False), ("step_normalized", True)])
def test_base_model_steps_as_the_reference(fx, tag, normalize):
    trainer, batch = U.step_setup(BaseModel, normalize)
    assert trainer.use_discriminator and isinstance(trainer.netD, DiscriminatorLoss)
    grid = int(fx["grid"])
    for call in range(2):
        losses, images = trainer(batch)
        keys = [str(k) for k in fx[f"{tag}_call{call}_loss_keys"]]
        assert sorted(losses) == keys
        got = np.array([float(losses[k].detach().mean()) for k in keys])
        np.testing.assert_allclose(got, fx[f"{tag}_call{call}_loss_values"], rtol=1e-5, err_msg=f"{tag} call {call} {keys}")
        names = sorted(k for k, _ in trainer.named_parameters())
        assert names == [str(k) for k in fx[f"{tag}_call{call}_param_keys"]]
        params = dict(trainer.named_parameters())
        flat = np.concatenate([params[k].detach().reshape(-1)[::grid].numpy() for k in names])
        np.testing.assert_allclose(flat, fx[f"{tag}_call{call}_params"], rtol=1e-4, atol=1e-7, err_msg=f"{tag} call {call}")
        rng = [float(images["PredImg"].detach().min()), float(images["PredImg"].detach().max())]
        np.testing.assert_allclose(rng, fx[f"{tag}_call{call}_pred_range"], rtol=1e-5, atol=1e-6)
        assert (rng[0] >= 0.0) == normalize                      # tanh's range moved to [0, 1] by normalize_image alone
    assert not np.array_equal(fx[f"{tag}_call0_params"], fx[f"{tag}_call1_params"])


def test_base_model_builds_and_refuses():
    trainer, batch = U.step_setup(BaseModel, False)
    with pytest.raises(NotImplementedError, match="num_steps = 2"):
        trainer(batch, num_steps=2)
    betas = lambda o: o.param_groups[0]["betas"]
    assert betas(trainer.optimizer_G) == betas(trainer.optimizer_D) == (0.0, 0.9)
    assert trainer.optimizer_G.param_groups[0]["lr"] == 5e-4 and trainer.optimizer_D.param_groups[0]["lr"] == 2e-3 and trainer.old_lr == 1e-3
    with pytest.raises(NotImplementedError, match="use_3_discrim"):
        BaseModel(U.OneConv(), U.train_opts(discriminator_losses="pix2pixHD", use_3_discrim=True))
    # isval: the model's own pair, the discriminator handed over, the images normalised
    seen = []
    model = U.OneConv()
    real = model.forward
    model.forward = lambda b, netD=None: (seen.append(netD), real(b, netD))[1]
    val = BaseModel(model, U.train_opts(discriminator_losses="pix2pixHD", normalize_image=True))
    before = [p.detach().clone() for p in val.parameters()]
    losses, images, back = val(batch, isval=True, return_batch=True)
    assert seen == [val.netD] and back is batch and set(losses) == {"L1", "Total Loss"} and float(images["PredImg"].min()) >= 0.0
    assert all(torch.equal(a, b) for a, b in zip(before, val.parameters()))
    # without a discriminator: Adam with betas (0.99, beta2) on the generator alone, and a step that moves it
    solo = BaseModel(U.OneConv(), U.train_opts())
    assert not solo.use_discriminator and solo.netD is None and not hasattr(solo, "optimizer_D") and betas(solo.optimizer_G) == (0.99, 0.9)
    w0 = solo.model.conv.weight.detach().clone()
    losses, _ = solo(batch)
    assert set(losses) == {"L1", "Total Loss"} and not torch.equal(w0, solo.model.conv.weight)
    # opt.init
    torch.manual_seed(0)
    inited = BaseModel(U.OneConv(), U.train_opts(init="normal"))
    assert float(inited.model.conv.bias.abs().max()) == 0.0 and 0.005 < float(inited.model.conv.weight.std()) < 0.04
    with pytest.raises(NotImplementedError, match="bogus"):
        BaseModel(U.OneConv(), U.train_opts(init="bogus"))


def test_compat_alias_leaves_the_other_tables_alone():
    tables = {n: dict(getattr(compat, n)) for n in ("ALIASES", "EVAL_ALIASES", "TRAINING_ALIASES", "GAN_ALIASES")}
    assert compat.BASE_MODEL_ALIASES == {"models.base_model": "pixelsynth_amd.base_model"}
    assert not any("models.base_model" in t for t in tables.values())
    import sys
    saved = {k: sys.modules.get(k) for k in ("models", "models.base_model")}
    try:
        sys.modules.pop("models.base_model", None)
        assert compat.install_base_model_aliases() == ["models.base_model"]
        from models.base_model import BaseModel as aliased
        assert aliased is BaseModel
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert tables == {n: dict(getattr(compat, n)) for n in tables}


def test_forward_train_assembles_the_loss_on_the_cpu():
    """no_outpainting (nothing of the AR path, which is on the device alone), the renderer replaced by a stand-in that keeps the graph"""
    opt = U.train_opts(no_outpainting=True, train_depth=True, vqvae=False)
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts
    torch.manual_seed(0)
    model = ZbufferModelPts(opt).train()
    assert model.vqvae is None
    bg = torch.zeros(1, 256, 256, dtype=torch.bool)
    bg[:, :, 200:] = True
    model.pts_transformer.forward_justpts = lambda src, pts, *a: (src * 0.5 + 0.01 * pts, bg)
    batch = U.make_batch(1)
    loss, out = model(batch)
    assert set(out) == U.OUTPUT_KEYS and set(loss) == {"L1", "Total Loss", "psnr", "ssim", "depth_loss"}
    depth = (out["PredDepthImg"] + 1) * 5
    assert float(depth.min()) >= U.MIN_Z - 1e-4 and float(depth.max()) <= U.MAX_Z + 1e-4 and not out["PredDepthImg"].requires_grad
    want = torch.nn.functional.l1_loss(out["PredImg"], batch["images"][-1]) + loss["depth_loss"]
    assert abs(float(loss["Total Loss"]) - float(want)) <= 1e-6 * float(want)
    assert abs(float(loss["depth_loss"]) - float((depth - batch["depths"][0]).abs().mean())) <= 1e-4
    assert torch.equal(out["ForegroundImg"], (~bg).float()[None])
    loss["Total Loss"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.pts_regressor.parameters())
    # every other setting goes where it went: 'train' alone reaches forward_train
    called = []
    model.forward_train = lambda b: called.append("train") or (None, {})
    model.forward_image = lambda b, netD=None: called.append("image") or (None, {})
    for setting in ("train", "gen_img", "gen_paired_img"):
        model.opt.model_setting = setting
        model(batch)
    assert called == ["train", "image", "image"]
    # without a VQ-VAE and with outpainting on: the reference's mixture-of-logistics branch, which is not built
    model2 = ZbufferModelPts(U.train_opts(vqvae=False)).train()
    model2.pts_transformer.forward_justpts = lambda src, pts, *a: (src, bg)
    with pytest.raises(NotImplementedError, match="mixture-of-logistics"):
        model2.forward_train(batch)
