"""Generate tests/golden/gan_train.npz by IMPORTING the reference (read-only), as make_golden.py does: the fixture holds seeds and the
reference's OUTPUTS only -- what its own DiscriminatorLoss (models/losses/gan_loss.py, models/networks/discriminators.py) in train() with
isTrain=True computes on the CPU for one generator step and then one discriminator step from freshly loaded weights:

  per size S in SIZES (two pairs of S x S images, fake = syn.image(FAKE_SEED + S, 2, 3, S), real = syn.image(REAL_SEED + S, 2, 3, S)):
    g_GAN, g_GAN_Feat, g_total        run_generator_one_step, then backward of its total:
    g_dfake                           the gradient to the fake image on an 8 x 8 grid, [:, :, ::S // 8, ::S // 8]
    g_grad_<i>_<name>                 the gradients of GRAD_KEYS of scale i, flattened, every GRID-th value
    g_u_<key>                         every weight_u after the step
    d_D_Fake, d_D_real, d_total       gradients zeroed, run_discriminator_one_step on the same pair, backward of its total:
    d_grad_<i>_<name>, d_u_<key>      as above

Run:  python tests/golden/make_gan_train.py
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from pixelsynth_amd import synthetic as syn  # noqa: E402

SIZES, WEIGHT_SEED, FAKE_SEED, REAL_SEED, GRID = (32, 64), 11, 100, 200, 29
GRAD_KEYS = ("model0.0.weight", "model2.0.0.weight_orig")


def train_opts():
    return argparse.Namespace(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=8, output_nc=3,
                              no_ganFeat_loss=False, isTrain=True, lambda_feat=10.0, lr=1e-4, niter=100, niter_decay=10)


def record(fx, tag, net):
    sd = dict(net.named_parameters())
    for i in range(2):
        for name in GRAD_KEYS:
            fx[f"{tag}_grad_{i}_{name}"] = sd[f"netD.netD.discriminator_{i}.{name}"].grad.reshape(-1)[::GRID].numpy().copy()
    for k, v in net.state_dict().items():
        if k.endswith("weight_u"):
            fx[f"{tag}_u_{k}"] = v.numpy().copy()


def main():
    from models.losses.gan_loss import DiscriminatorLoss
    torch.set_num_threads(8)
    fx = {}
    for S in SIZES:
        with contextlib.redirect_stdout(io.StringIO()):
            net = DiscriminatorLoss(train_opts()).train()
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, WEIGHT_SEED).items()}, strict=True)
        fake = torch.from_numpy(syn.image(FAKE_SEED + S, 2, 3, S)).requires_grad_()
        real = torch.from_numpy(syn.image(REAL_SEED + S, 2, 3, S))
        g = net.run_generator_one_step(fake, real)
        g["Total Loss"].mean().backward()
        tag = f"s{S}_g"
        fx[f"{tag}_GAN"], fx[f"{tag}_GAN_Feat"], fx[f"{tag}_total"] = (g[k].detach().reshape(-1).numpy().copy() for k in ("GAN", "GAN_Feat", "Total Loss"))
        fx[f"{tag}_dfake"] = fake.grad[:, :, ::S // 8, ::S // 8].numpy().copy()
        record(fx, tag, net)
        net.zero_grad()
        d = net.run_discriminator_one_step(fake.detach(), real)
        d["Total Loss"].mean().backward()
        tag = f"s{S}_d"
        fx[f"{tag}_D_Fake"], fx[f"{tag}_D_real"], fx[f"{tag}_total"] = (d[k].detach().reshape(-1).numpy().copy() for k in ("D_Fake", "D_real", "Total Loss"))
        record(fx, tag, net)
        maps = net.netD.netD(torch.cat([fake.detach(), real], 0))       # (a third forward, after everything is recorded: the shapes only)
        print(S, "GAN", fx[f"s{S}_g_GAN"], "GAN_Feat", fx[f"s{S}_g_GAN_Feat"], "D total", fx[f"s{S}_d_total"],
              [tuple(t.shape) for t in maps[1]])
    fx["sizes"], fx["weight_seed"], fx["fake_seed"], fx["real_seed"], fx["grid"] = (np.array(v) for v in (SIZES, WEIGHT_SEED, FAKE_SEED, REAL_SEED, GRID))
    np.savez_compressed(os.path.join(HERE, "gan_train.npz"), **fx)
    print("gan_train.npz", len(fx), "arrays,", os.path.getsize(os.path.join(HERE, "gan_train.npz")), "bytes")


if __name__ == "__main__":
    main()
