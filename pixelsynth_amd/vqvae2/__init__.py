from .vqvae import VQVAETop, Quantize, vqvae_train  # noqa: F401
