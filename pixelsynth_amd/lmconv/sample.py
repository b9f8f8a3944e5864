"""Autoregressive sampling over the 32x32 code grid -- drop-in for the reference's
models/lmconv/sample.py:sample() (same signature, same return value).

Three evaluation modes (args.ar_mode or env PS_AR_MODE):
  "fused"       (default) the whole loop runs on the device through ps_pixelcnn_ar_run: exact
                incremental evaluation (one network COLUMN per location against cached activations,
                all columns of a dependency level in one launch) and an inverse-CDF categorical draw from
                softmax(logits/T) with uniforms taken from torch's generator after the reference's
                seeding rule.  Same distribution as the reference, different RNG stream.
  "multinomial" the incremental evaluation, but every draw is torch.multinomial called exactly as
                the reference calls it (1 + seed draws per position, sample.py:61-63).
  "reference"   the reference's loop verbatim: one FULL network forward per sampled position.
All three produce the same logits at every decided position (the masks only admit earlier locations,
so a location's activations never change once computed -- SURVEY.md 7).
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ar_plan import plan_from_reference_args


def _sample_indices(generation_idx, background_mask, obs):
    """sample.py:23-41: per image, the positions with background_mask == 1 in generation order."""
    out = []
    bm = background_mask.detach().cpu().numpy()
    for image_number in range(bm.shape[0]):
        sel = [[int(i), int(j)] for i, j in generation_idx[image_number] if bm[image_number, int(i), int(j)] == 1]
        out.append(np.array(sel, dtype=np.int64).reshape(-1, 2))
    return out


def sample(model, generation_idx, mask_init, mask_undilated, mask_dilated, batch_to_complete, obs, args, seed=0,
           temperature=1.0, background_mask=None):
    mode = getattr(args, "ar_mode", None) or os.environ.get("PS_AR_MODE", "fused")
    num_classes = args.num_classes
    batch_to_complete_full = torch.clone(batch_to_complete)
    dev = torch.device("cuda", torch.cuda.current_device())
    B = batch_to_complete.shape[0]
    H, W = int(obs[1]), int(obs[2])
    L = H * W

    np.random.seed(seed)
    seed2 = seed * 10 + np.random.randint(188)          # sample.py:13-15
    torch.manual_seed(seed2)
    model.eval()

    codes = batch_to_complete.to(dev).to(torch.int64).clone()

    if mode == "reference":
        sample_indices = _sample_indices(generation_idx, background_mask, obs)
        data = F.one_hot(codes, num_classes).permute(0, 3, 1, 2).to(torch.float32)
        for b in range(B):
            if len(sample_indices[b]) > 0:
                data[b, :, sample_indices[b][:, 0], sample_indices[b][:, 1]] = 0      # sample.py:47
        for n_pix in range(len(sample_indices[0])):                                    # sample.py:54
            out = model([data, mask_init, mask_undilated, mask_dilated], sample=True)
            for b in range(out.shape[0]):
                (i, j) = sample_indices[b][n_pix]
                prob = torch.softmax(out[:, :, i, j] / temperature, 1)
                new_samples = torch.multinomial(prob, 1).squeeze(-1)
                for _ in range(seed):
                    new_samples = torch.multinomial(prob, 1).squeeze(-1)
                data[b, :, i, j] = F.one_hot(new_samples[b], num_classes).to(torch.float32)
    else:
        eng = model.engine(H, W, B)
        plan = plan_from_reference_args(generation_idx[:B], (mask_init, mask_undilated, mask_dilated), background_mask[:B], dev)
        masks = (plan.mask_init, plan.mask_undilated, plan.mask_dilated)
        c32 = codes.view(B, L).to(torch.int32).contiguous()
        if mode == "fused":
            uniforms = torch.rand(B, L, device=dev, dtype=torch.float32)
            eng.ar_run(c32, plan.order_loc, plan.region, *masks, temperature=temperature, uniforms=uniforms,
                       first_step=plan.first_step, waves=plan.waves)
            eng.check()   # a column launch that gave up on an in-launch wait raises here instead of returning wrong codes
        elif mode == "multinomial":
            region_np = plan.region.cpu().numpy()
            c32[plan.region.bool()] = -1
            for step in range(plan.first_step, L):
                logits = eng.ar_step(c32, plan.order_loc, *masks, step, plan.first_step)
                for b in range(B):
                    q = int(plan.order_host[b, step])
                    if not region_np[b, q]:
                        continue
                    prob = torch.softmax(logits / temperature, 1)
                    new_samples = torch.multinomial(prob, 1).squeeze(-1)
                    for _ in range(seed):
                        new_samples = torch.multinomial(prob, 1).squeeze(-1)
                    c32[b, q] = new_samples[b].to(torch.int32)
            eng.check()
        else:
            raise ValueError(f"unknown AR mode {mode!r}")
        data = F.one_hot(c32.view(B, H, W).to(torch.int64), num_classes).permute(0, 3, 1, 2).to(torch.float32)

    loss_score = nn.CrossEntropyLoss()(data, batch_to_complete_full.to(dev).to(torch.int64))
    # revert seeding for dataloader (sample.py:70-71)
    torch.manual_seed(args.dataloader_seed)
    np.random.seed(args.dataloader_seed)
    return data, loss_score
