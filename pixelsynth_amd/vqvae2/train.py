"""One optimisation step of the VQ-VAE (the inner loop of the reference's train_vqvae.py): reconstruction error plus the weighted
commitment term.  The quantisers update their codebooks inside the forward pass (vqvae2/vqvae.py: Quantize.forward in train() mode, on
csrc/vq_train.hip); everything else learns through the optimiser -- under vqvae_train("hip") through the convolutions of
vqvae2/conv_train.py, under the default vqvae_train("torch") through torch's."""
from torch.nn import functional as F

from ..networks.f16x3 import check_f16x3_overflow, flag
from .vqvae import vqvae_train


def train_step(model, optimizer, img, latent_loss_weight=0.25):
    """model in train() mode, img (B, 3, H, W) float32 on the device -> (reconstruction loss, latent loss) as Python floats, after
    one step of `optimizer` on  mse(model(img)[0], img) + latent_loss_weight * mean(latent loss).
    Under vqvae_train("hip") the split-fp16 convolutions' overflow flag is cleared before the forward pass and read after the backward
    pass (one synchronisation, which the return values need anyway): an activation beyond fp16's range raises RuntimeError BEFORE
    optimizer.step(), so no parameter moves on wrong gradients.  The codebooks' EMA update of that forward pass has already happened
    by then -- it is part of Quantize.forward -- and is not undone."""
    hip = vqvae_train.resolve() == "hip" and img.is_cuda
    optimizer.zero_grad()
    if hip:
        flag(img.device).zero_()
    out, latent = model(img)
    recon = F.mse_loss(out, img)
    latent = latent.mean()
    (recon + latent_loss_weight * latent).backward()
    if hip:
        check_f16x3_overflow(img.device)
    optimizer.step()
    return float(recon.detach()), float(latent.detach())
