"""One optimisation step of the VQ-VAE (the inner loop of the reference's train_vqvae.py): reconstruction error plus the weighted
commitment term.  The quantisers update their codebooks inside the forward pass (vqvae2/vqvae.py: Quantize.forward in train() mode, on
csrc/vq_train.hip); everything else learns through the optimiser."""
from torch.nn import functional as F


def train_step(model, optimizer, img, latent_loss_weight=0.25):
    """model in train() mode, img (B, 3, H, W) float32 on the device -> (reconstruction loss, latent loss) as Python floats, after
    one step of `optimizer` on  mse(model(img)[0], img) + latent_loss_weight * mean(latent loss)."""
    optimizer.zero_grad()
    out, latent = model(img)
    recon = F.mse_loss(out, img)
    latent = latent.mean()
    (recon + latent_loss_weight * latent).backward()
    optimizer.step()
    return float(recon.detach()), float(latent.detach())
