"""Inference mirror of the reference's models/losses/gan_loss.py for what the novel-view path calls:
`netD.run_discriminator_one_step(pred, real)["D_Fake"]` (models/z_buffermodel.py:254) -- the discriminator-side GAN loss of the
multiscale discriminator on a candidate.  Same class names and state_dict layout (`netD.netD.discriminator_<i>...`).

With opt.isTrain (the reference's train options) it is the training mirror as well: run_generator_one_step (hinge + feature matching,
a gradient to the fake image), run_discriminator_one_step with gradients to the discriminator's parameters, get_optimizer, and
adversarial_step -- one optimiser step of both sides as models/base_model.py takes it.  With opt.isTrain false everything is as before."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..networks import discriminators, gan_train


class GANLoss(nn.Module):
    """gan_loss.py:20-113: hinge (default), ls, original or wgan loss of a prediction or of the list of lists a multiscale
    discriminator returns (the last entry of every scale counts; the mean over scales)."""

    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0, tensor=torch.FloatTensor, opt=None):
        super().__init__()
        if gan_mode not in ("ls", "original", "w", "hinge"):
            raise ValueError("Unexpected gan_mode {}".format(gan_mode))
        self.real_label, self.fake_label, self.gan_mode, self.opt = target_real_label, target_fake_label, gan_mode, opt

    def loss(self, input, target_is_real, for_discriminator=True):
        if self.gan_mode in ("original", "ls"):
            target = torch.full_like(input, self.real_label if target_is_real else self.fake_label)
            return F.binary_cross_entropy_with_logits(input, target) if self.gan_mode == "original" else F.mse_loss(input, target)
        if self.gan_mode == "hinge":
            if for_discriminator:
                return -torch.mean(torch.min((input if target_is_real else -input) - 1, torch.zeros_like(input)))
            assert target_is_real, "The generator's hinge loss must be aiming for real"
            return -torch.mean(input)
        return -input.mean() if target_is_real else input.mean()

    def __call__(self, input, target_is_real, for_discriminator=True):
        if isinstance(input, list):
            loss = 0
            for pred_i in input:
                if isinstance(pred_i, list):
                    pred_i = pred_i[-1]
                loss_tensor = self.loss(pred_i, target_is_real, for_discriminator)
                bs = 1 if len(loss_tensor.size()) == 0 else loss_tensor.size(0)
                loss = loss + torch.mean(loss_tensor.view(bs, -1), dim=1)
            return loss / len(input)
        return self.loss(input, target_is_real, for_discriminator)


class BaseDiscriminator(nn.Module):
    """gan_loss.py:116-238: fake and real go through D in one batch.  Inference (opt.isTrain false): discriminator mode under no_grad,
    D_Fake / D_real / Total Loss.  Training: both modes, with their graphs."""

    def __init__(self, opt, name):
        super().__init__()
        if name == "pix2pixHD":
            self.netD = discriminators.define_D(opt)
        self.criterionGAN = GANLoss(opt.gan_mode, opt=opt)
        self.opt = opt

    def discriminate(self, fake_image, real_image):
        out = self.netD(torch.cat([fake_image, real_image], dim=0))
        fake = [[t[: t.size(0) // 2] for t in p] for p in out]
        real = [[t[t.size(0) // 2:] for t in p] for p in out]
        return fake, real

    @torch.no_grad()
    def score(self, fake_image, real_image, mode="discriminator"):
        """The inference form (opt.isTrain false): no graph, discriminator mode only"""
        if mode != "discriminator":
            raise NotImplementedError("the inference mirror scores candidates (discriminator mode); training is out of scope")
        pred_fake, pred_real = self.discriminate(fake_image, real_image)
        losses = {"D_Fake": self.criterionGAN(pred_fake, False, for_discriminator=True),
                  "D_real": self.criterionGAN(pred_real, True, for_discriminator=True)}
        losses["Total Loss"] = sum(losses.values()).mean()
        return losses

    def compute_discrimator_loss(self, fake_image, real_image):
        """gan_loss.py:172-189 (its spelling): the fake image detached, gradients to the discriminator's parameters"""
        fake_image = fake_image.detach().requires_grad_()
        pred_fake, pred_real = self.discriminate(fake_image, real_image)
        losses = {"D_Fake": self.criterionGAN(pred_fake, False, for_discriminator=True),
                  "D_real": self.criterionGAN(pred_real, True, for_discriminator=True)}
        losses["Total Loss"] = sum(losses.values()).mean()
        return losses

    def compute_generator_loss(self, fake_image, real_image):
        """gan_loss.py:191-218: the hinge term aiming for real and, unless no_ganFeat_loss, the L1 between the fake and the (detached)
        real halves of every intermediate map, lambda_feat / num_D each -- all maps through gan_train.feature_matching"""
        out = self.netD(torch.cat([fake_image, real_image], dim=0))
        pred_fake = [[t[: t.size(0) // 2] for t in p] for p in out]
        losses = {"GAN": self.criterionGAN(pred_fake, True, for_discriminator=False)}
        if not self.opt.no_ganFeat_loss:
            maps = [t for p in out for t in p[:-1]]         # (the last output of a scale is its prediction)
            losses["GAN_Feat"] = gan_train.feature_matching(maps, self.opt.lambda_feat / len(out), self.opt)
        losses["Total Loss"] = sum(losses.values()).mean()
        return losses

    def forward(self, fake_image, real_image, mode="discriminator"):
        if not getattr(self.opt, "isTrain", False):
            return self.score(fake_image, real_image, mode)
        if mode == "generator":
            return self.compute_generator_loss(fake_image, real_image)
        if mode == "discriminator":
            return self.compute_discrimator_loss(fake_image, real_image)
        raise ValueError(f"mode = {mode!r}: 'generator' or 'discriminator'")


class DiscriminatorLoss(nn.Module):
    """gan_loss.py:241-288: what train / demo hand to the model as `netD`."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.netD = BaseDiscriminator(opt, name=opt.discriminator_losses)

    def get_optimizer(self):
        # (the reference writes betas=(0, 0.9); torch now insists on two floats)
        return torch.optim.Adam(list(self.netD.parameters()), lr=self.opt.lr * 2, betas=(0.0, 0.9))

    def run_generator_one_step(self, pred_img, gt_img):
        return self.netD(pred_img, gt_img, mode="generator")

    def run_discriminator_one_step(self, pred_img, gt_img):
        return self.netD(pred_img, gt_img, mode="discriminator")


def adversarial_step(netD, optimizer_G, optimizer_D, t_losses, pred_img, gt_img):
    """One optimiser step of generator and discriminator, the reference's BaseModel.__call__ (models/base_model.py:105-134) for
    num_steps = 1: t_losses are the generator's image losses on pred_img (still attached to its graph), netD a DiscriminatorLoss built
    with opt.isTrain.  The generator's backward over t_losses["Total Loss"] + g_losses["Total Loss"] and its step; then the
    discriminator's zero_grad, loss on the detached prediction, backward and step.  -> t_losses with the GAN terms of both merged in,
    their two totals left out (t_losses' own total stays)."""
    optimizer_G.zero_grad()
    g_losses = netD.run_generator_one_step(pred_img, gt_img)
    (g_losses["Total Loss"] + t_losses["Total Loss"]).mean().backward()
    optimizer_G.step()
    optimizer_D.zero_grad()
    d_losses = netD.run_discriminator_one_step(pred_img, gt_img)
    d_losses["Total Loss"].mean().backward()
    optimizer_D.step()
    g_losses.pop("Total Loss")
    d_losses.pop("Total Loss")
    merged = dict(t_losses)
    merged.update(g_losses)
    merged.update(d_losses)
    return merged
