"""What a training loop of the generator needs beside the model (z_buffermodel.ZbufferModelPts.forward_train) and the step
(base_model.BaseModel): the route switches of the training kernels as one context.

Several of the training units are opt-in (their switches default to the torch formula, so that a model trained before they existed
computes what it computed); hip_routes() turns all of them on for the calls inside."""
import contextlib

from .lmconv.train_ops import pixelcnn_train
from .networks.block_train import decoder_block_train
from .networks.disc_conv import discriminator_conv_train
from .networks.f16x3 import decoder_conv_train
from .networks.spectral_train import spectral_train
from .networks.thin_train import decoder_thin_train
from .networks.train_glue import train_glue
from .networks.unet_train import unet_train

# every training switch and its HIP value (routing.Switch); the norm's and the discriminator's switches default to "hip" already
HIP_ROUTES = ((decoder_conv_train, "f16x3"), (decoder_block_train, "hip"), (decoder_thin_train, "hip"), (pixelcnn_train, "hip"),
              (train_glue, "hip"))


@contextlib.contextmanager
def hip_routes():
    """Every training switch at its HIP value for the calls inside, whatever the options and the environment say: decoder_conv_train
    ("f16x3"), decoder_block_train, decoder_thin_train, pixelcnn_train, train_glue ("hip").  Blocks nest like the switches' own: a
    switch forced inside this block wins there.  -> {switch name: mode} as Switch.forced() reports them inside the block."""
    with contextlib.ExitStack() as stack:
        for switch, value in HIP_ROUTES:
            stack.enter_context(switch(value))
        yield {switch.name: switch.forced() for switch, _ in HIP_ROUTES}


@contextlib.contextmanager
def hip_routes_with_discriminator():
    """hip_routes() and, on top, discriminator_conv_train("f16"): the 4 x 4 convolutions of the discriminator's model1..3 through
    networks/disc_conv.py as well -- exactly `with hip_routes(), discriminator_conv_train("f16"):`.  That switch is not one of HIP_ROUTES
    (its default is "torch").  -> hip_routes()'s dict with the sixth switch added."""
    with hip_routes() as forced, discriminator_conv_train("f16"):
        yield dict(forced, **{discriminator_conv_train.name: discriminator_conv_train.forced()})


@contextlib.contextmanager
def hip_routes_with_spectral(discriminator=False):
    """hip_routes() -- or, with `discriminator`, hip_routes_with_discriminator() -- and, on top, spectral_train("hip"): the spectral
    normalisation of the decoder's, the Unet's and the discriminator's layers as one batched pass per forward (networks/spectral_train.py).
    That switch is not one of HIP_ROUTES either (its default is "torch").  -> the inner context's dict with this switch added."""
    with (hip_routes_with_discriminator() if discriminator else hip_routes()) as forced, spectral_train("hip"):
        yield dict(forced, **{spectral_train.name: spectral_train.forced()})


@contextlib.contextmanager
def hip_routes_with_unet(discriminator=False):
    """hip_routes_with_spectral(discriminator) and, on top, unet_train("hip"): the depth Unet's batch norms, skip joins and wide 3 x 3
    convolutions through networks/unet_train.py and conv_routes._unet_train_conv.  That switch is not one of HIP_ROUTES either (its
    default is "torch").  -> the inner context's dict with this switch added."""
    with hip_routes_with_spectral(discriminator) as forced, unet_train("hip"):
        yield dict(forced, **{unet_train.name: unet_train.forced()})
