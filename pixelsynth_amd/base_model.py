"""The training step of the generator -- counterpart of the reference's models/base_model.py:BaseModel: the model, the discriminator's
loss module, their two Adam optimisers, and __call__, one optimiser step of both sides on a batch (or, with isval, the model's own
forward).  The same constructor, attribute names (model, netD, optimizer_G, optimizer_D, use_discriminator) and return values.

    model = ZbufferModelPts(opt)                   # opt.model_setting = "train", opt.losses, opt.isTrain, ...
    trainer = BaseModel(model, opt)
    losses, images = trainer(batch)                # forward_train, backward, both optimisers' steps

The adversarial step itself is losses.gan_loss.adversarial_step, which the discriminator's tests pin against the reference; the HIP routes
of the training kernels that are opt-in are turned on around the call with training.hip_routes():

    with training.hip_routes():
        losses, images = trainer(batch)

TRAIN UNDER IT.  At their defaults the opt-in switches leave the decoder's pooled joins to torch, whose F.avg_pool2d backward is wrong for
channels-last operands on the ROCm stack this was measured on (tools/avg_pool_bwd_check.py prints the figures: 0.8 absolute on randn); the
gradients of the decoder's Down blocks and of everything in front of them -- the Unet's included -- are then off by 1 % to 70 %.  The
project's own adjoint (decoder_block_train("hip"), which hip_routes() turns on) agrees with the host.  BaseModel does not force the routes
itself: a switch is the caller's to set, and the defaults are what every earlier caller of the decoder got.

Not built: num_steps != 1 (the reference marks it "not fully implemented": its loop divides by the weight where it means to multiply)
and opt.use_3_discrim (two further discriminators the reference constructs and never steps)."""
import torch
import torch.nn as nn
from torch.nn import init

from .losses.gan_loss import DiscriminatorLoss, adversarial_step


class BaseModel(nn.Module):
    def __init__(self, model, opt):
        super().__init__()
        self.model = model
        self.opt = opt
        if getattr(opt, "discriminator_losses", None):      # base_model.py:15-33
            if getattr(opt, "use_3_discrim", False):
                raise NotImplementedError("BaseModel: opt.use_3_discrim is not built (the reference never steps its two extra discriminators)")
            self.use_discriminator = True
            self.netD = DiscriminatorLoss(opt)
            if opt.isTrain:
                self.optimizer_D = torch.optim.Adam(list(self.netD.parameters()), lr=opt.lr_d, betas=(opt.beta1, opt.beta2))
                self.optimizer_G = torch.optim.Adam(list(self.model.parameters()), lr=opt.lr_g, betas=(opt.beta1, opt.beta2))
        else:                                                # :34-40
            self.use_discriminator = False
            self.netD = None
            self.optimizer_G = torch.optim.Adam(list(self.model.parameters()), lr=opt.lr_g, betas=(0.99, opt.beta2))
        if opt.isTrain:
            self.old_lr = opt.lr
        if getattr(opt, "init", None):
            self.init_weights()

    def init_weights(self, gain=0.02):
        """base_model.py:48-79: every module whose class name has Conv or Linear in it and that has a weight, by opt.init"""
        def init_func(m):
            classname = m.__class__.__name__
            if hasattr(m, "weight") and (classname.find("Conv") != -1 or classname.find("Linear") != -1):
                kind = self.opt.init
                if kind == "normal":
                    init.normal_(m.weight.data, 0.0, gain)
                elif kind == "xavier":
                    init.xavier_normal_(m.weight.data, gain=gain)
                elif kind == "xavier_uniform":
                    init.xavier_uniform_(m.weight.data, gain=1.0)
                elif kind == "kaiming":
                    init.kaiming_normal_(m.weight.data, a=0, mode="fan_in")
                elif kind == "orthogonal":
                    init.orthogonal_(m.weight.data)
                else:
                    raise NotImplementedError("initialization method [%s] is not implemented" % kind)
                if hasattr(m, "bias") and m.bias is not None:
                    init.constant_(m.bias.data, 0.0)

        self.apply(init_func)
        for m in self.children():       # propagate to children
            if hasattr(m, "init_weights"):
                m.init_weights(self.opt.init, gain)

    def _normalized(self, output_images):
        """opt.normalize_image: every *Img output from [-1, 1] to [0, 1], in place in the dict (base_model.py:96-99, :143-146)"""
        if getattr(self.opt, "normalize_image", False):
            for k in output_images.keys():
                if "Img" in k:
                    output_images[k] = 0.5 * output_images[k] + 0.5
        return output_images

    def __call__(self, batch, isval=False, num_steps=1, return_batch=False):
        """base_model.py:81-148.  isval: the model's forward with the discriminator handed over -> (losses, images[, batch]).  Otherwise one
        optimiser step: model(batch), then with a discriminator gan_loss.adversarial_step -- the generator's backward over its image
        losses plus the GAN terms and its step, the discriminator's backward on the detached prediction and its step -- -> (the merged
        losses, images).  Without a discriminator the reference stops in a debugger (:136-137) and would then read a `dataloader` it
        does not have; zero_grad, the backward of "Total Loss" and the generator's step is THIS project's reading of that branch."""
        if isval:
            t_losses, output_images = self.model(batch, self.netD)
            self._normalized(output_images)
            return (t_losses, output_images, batch) if return_batch else (t_losses, output_images)
        if num_steps != 1:
            raise NotImplementedError(f"BaseModel: num_steps = {num_steps}: one discriminator step per generator step is what is built "
                                      "(the reference marks more as not fully implemented)")
        if self.use_discriminator:
            t_losses, output_images = self.model(batch)
            t_losses = adversarial_step(self.netD, self.optimizer_G, self.optimizer_D, t_losses, output_images["PredImg"],
                                        output_images["OutputImg"])
        else:
            self.optimizer_G.zero_grad()
            t_losses, output_images = self.model(batch)
            t_losses["Total Loss"].mean().backward()
            self.optimizer_G.step()
        return t_losses, self._normalized(output_images)
