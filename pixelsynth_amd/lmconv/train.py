"""One optimisation step of the PixelCNN on given codes: the inner loop of the reference's train_lmconv.py:704-733 for accum_freq = 1
(zero_grad, the mean cross entropy of the codes in their generation order, backward, gradient clipping, optimizer step).  The loss is
likelihood.ar_loss, so the route is its: the masked convolutions on HIP both ways, and under pixelcnn_train("hip") (train_ops.py) the
passes between them and the loss's backward as well.  Nothing comes down to the host."""
import math

import torch

from ..likelihood import ar_loss


def train_step(model, optimizer, codes, plan_or_masks, region=None, group="all", clip=None, temperature=1.0):
    """model: ZbufferModelPts (its outpaint2 is trained) or OurPixelCNN; optimizer: one over the parameters to tune; codes,
    plan_or_masks, region, group, temperature: as ar_loss takes them; clip: the largest norm of the gradient over all the model's
    parameters (clip_grad_norm_), None or <= 0: no clipping.
    -> (loss, bits_per_code, grad_norm): 0-dim device tensors, detached; grad_norm is the norm BEFORE clipping, None without clipping."""
    net = getattr(model, "outpaint2", model)
    optimizer.zero_grad()
    loss = ar_loss(model, codes, plan_or_masks, region=region, group=group, temperature=temperature)
    loss.backward()
    grad_norm = None
    if clip is not None and clip > 0:
        grad_norm = torch.nn.utils.clip_grad_norm_(net.parameters(), clip).detach()
    optimizer.step()
    loss = loss.detach()
    return loss, loss / math.log(2.0), grad_norm
