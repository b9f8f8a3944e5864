"""What the tests of the training step's glue kernels (csrc/train_glue.hip, networks/train_glue.py) compare against: the fp64 formulas
of include/pixelsynth_train_glue.h and the depth head's bounds.

combine_mask_nhwc has no bound: its arithmetic is the torch formula's (two products and one addition per value, each rounded on its
own), so forward and backward are compared bit for bit against that formula on the device.

The depth head.  u = 2^-24 bounds the relative error of one fp32 rounding; s = sigmoid(raw) comes with a relative error of C_SIG u --
tests/_pixelcnn_train_ref.py's constant, measured there on torch's own fp32 sigmoid over 0.3 + 1.5 randn and the +-30 case, the values
drawn here too -- and the fp64 reference is evaluated with the constants as the caller gave them (doubles), so the rounding of
float(max_z - min_z), float(min_z) and 0.01f counts as well:

  range    depth = fl(fl(s R) + lo), R = max_z - min_z, lo = min_z.  s's error C_SIG u s |R|, R's rounding u s |R|, the product's
           u s |R|, lo's rounding u |lo|, the addition's u |depth|:
                                                    |depth - depth64| <= ((C_SIG + 2) u s |R| + u |lo| + u |depth64|) SLACK
  inverse  b = fl(fl(10 s) + 0.01f): s's error and the product's (C_SIG + 1) u 10 s, 0.01f's rounding u 0.01, the addition's u b;
           depth = fl(1 / b), and d(1 / b) = -db / b^2 (b >= 0.01 and db / b <= 7 u: the second-order term is inside SLACK):
                                                    |depth - depth64| <= (((C_SIG + 1) u 10 s + u 0.01 + u b) / b^2 + u depth64) SLACK
  pred_img = fl(fl(depth / 5) - 1), a true division: compared BIT FOR BIT against the same two operations on the kernel's own depth,
           evaluated on the host (numpy float32, IEEE division) -- torch's device kernel multiplies by the rounded reciprocal of a
           scalar divisor and may differ in the last bit, which is why the host is the reference here.
  g        the project's rule for gradients: |g - g64| <= 4 max(E32, 1e-6 max |g64|), E32 the largest error of torch's fp32 evaluation
           of the same formula on the host (grad_bound); no element is left out.
"""
import numpy as np
import torch

from _pixelcnn_train_ref import C_SIG, SLACK, U, autograd, check, grad_bound  # noqa: F401  (the tests import them from here)

RANGE, INVERSE = 0, 1                      # PS_GLUE_DEPTH_* of the header
MIN_Z, MAX_Z = 0.5, 10.0                   # the tests' range (the reference's RealEstate10K options: min_z 0.5 ... max_z 10)


def raws(shape, kind, seed=0):
    """The regressor outputs the tests draw: "randn" = 0.3 + 1.5 randn, "large" = +-30 with random signs plus randn"""
    gen = torch.Generator().manual_seed(seed)
    x = 0.3 + 1.5 * torch.randn(shape, generator=gen)
    if kind == "large":
        x = 30.0 * torch.sign(torch.randn(shape, generator=gen)) + torch.randn(shape, generator=gen)
    return x


def depth_formula(raw, mode, min_z=MIN_Z, max_z=MAX_Z):
    """The reference's depth rule (z_buffermodel.py:303-314) in raw's dtype"""
    s = torch.sigmoid(raw)
    return 1. / (s * 10 + 0.01) if mode == INVERSE else s * (max_z - min_z) + min_z


def depth_bound(raw, mode, min_z=MIN_Z, max_z=MAX_Z):
    """-> (depth64, the bound on |depth - depth64|), both fp64 of raw's shape (docstring)"""
    x = raw.double().cpu()
    s = torch.sigmoid(x)
    d64 = depth_formula(x, mode, min_z, max_z)
    if mode == INVERSE:
        b = s * 10 + 0.01
        return d64, (((C_SIG + 1) * U * 10 * s + U * 0.01 + U * b) / (b * b) + U * d64.abs()) * SLACK
    return d64, ((C_SIG + 2) * U * s * abs(max_z - min_z) + U * abs(min_z) + U * d64.abs()) * SLACK


def pred_img_host(depth):
    """fl(fl(depth / 5) - 1) of an fp32 depth in IEEE fp32 on the host -> a float32 tensor"""
    d = depth.detach().cpu().numpy().astype(np.float32)
    return torch.from_numpy((d / np.float32(5.0) - np.float32(1.0)).astype(np.float32))


def combine_formula(gen_fs, input_gt, background_mask):
    """get_combined (z_buffermodel.py:703-708) and the decoder's torch.cat with the mask channel, written out: (B,C+1,H,W) NCHW"""
    b, h, w = background_mask.shape
    fg = (~background_mask).float().to(gen_fs.dtype)
    bg = background_mask.float().to(gen_fs.dtype)
    combined = gen_fs * fg.view(b, -1, h, w) + input_gt * bg.view(b, -1, h, w)
    return torch.cat((combined, fg.unsqueeze(1)), 1)


def same_bits(a, b):
    """Whether two fp32 tensors hold the same bits (NaN payloads and the sign of zero included)"""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
