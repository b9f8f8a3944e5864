"""What the tests of the VQ-VAE's training convolutions (csrc/vq_conv_train.hip, vqvae2/conv_train.py; test_vq_conv_train_cpu.py,
test_vq_conv_train_gpu.py) compare against: the mirror of the split into parts of include/pixelsynth_vq_conv_train.h, Python mirrors of
the two folds, the fp64 formulas of the ends, the equivalent 3 x 3 problems of the stride-2 forms (folded and masked as the kernels do) for
the two rules of tests/_conv_bwd_ref.py, and fp64 / fp32 twins of the encoder and the decoder whose ReLU decisions are given.  No test in
here.

Bounds (none is new):  rules 1 and 2 of _conv_bwd_ref.check;  the chain bound 1.01 (L + parts) 2^-24 sum |g| |x| of _thin_train_ref
(L = the most pixels a group accumulates plus the groups added after it);  the gather bound 1.01 n 2^-24 sum |w g| of _block_train_ref
(n = 48 terms of the head's input gradient)."""
import torch
import torch.nn.functional as F

import _conv_bwd_ref as cref
from pixelsynth_amd.vqvae2.vqvae import _d2s, _s2d, convt_weight, s2d_weight

U = 2.0 ** -24
MAX_PARTS, MIN_PART, GROUPS = 256, 256, 16       # PS_VQ_CONV_TRAIN_* of the header (tests/test_vq_conv_train_cpu.py holds them to it)
SLAB = 64 * 48 + 2 * 64                          # floats of a part's slab


# ---- the split of the pixels ---------------------------------------------------------------------------------------------------------
def part_ranges(P):
    part = max(MIN_PART, GROUPS * -(-(-(-P // GROUPS)) // MAX_PARTS))
    return [(p, min(P, p + part)) for p in range(0, P, part)]


def chain(P):
    return max(-(-(hi - lo) // GROUPS) for lo, hi in part_ranges(P)) + GROUPS


def workspace_bytes(P):
    return -(-(len(part_ranges(P)) * SLAB * 4) // 256) * 256


# ---- the folds: the inverses of s2d_weight / convt_weight on their live positions ---------------------------------------------------------
BY, SY, DY = (0, 1, 1, 2), (1, 0, 1, 0), (2, 1, 1, 0)


def fold(w3):
    """(Co, 4 Ci, 3, 3) -> (Co, Ci, 4, 4)"""
    Co, Ci = w3.size(0), w3.size(1) // 4
    v = w3.reshape(Co, 2, 2, Ci, 3, 3)
    out = w3.new_zeros(Co, Ci, 4, 4)
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky, kx] = v[:, SY[ky], SY[kx], :, BY[ky], BY[kx]]
    return out


def fold_t(w3):
    """(4 Co, Ci, 3, 3) -> (Ci, Co, 4, 4)"""
    Co, Ci = w3.size(0) // 4, w3.size(1)
    v = w3.reshape(2, 2, Co, Ci, 3, 3)
    out = w3.new_zeros(Ci, Co, 4, 4)
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky, kx] = v[SY[ky], SY[kx], :, :, DY[ky], DY[kx]].transpose(0, 1)
    return out


def fold_kernel_layout(g, transposed):
    """The kernel's own operand layouts: (Co, 3, 3, 4 Ci) -> (Co, Ci, 4, 4) / (4 Co, 3, 3, Ci) -> (Ci, Co, 4, 4)"""
    return (fold_t if transposed else fold)(g.permute(0, 3, 1, 2))


# ---- the ends --------------------------------------------------------------------------------------------------------------------------
def ends_dw(img, wide):
    """dW[o, c, ky, kx] = sum wide[b, o, y, x] * img[b, c, 2 y - 1 + ky, 2 x - 1 + kx]; img (B, 3, H, W), wide (B, 64, H / 2, W / 2)"""
    cols = F.unfold(img, 4, padding=1, stride=2)                       # (B, 48, L), rows (c, ky, kx)
    return torch.einsum("bol,bkl->ok", wide.reshape(wide.size(0), 64, -1), cols).reshape(64, 3, 4, 4)


def ends_bound(img, wide):
    P = wide.size(0) * wide.size(2) * wide.size(3)
    return 1.01 * (chain(P) + len(part_ranges(P))) * U * ends_dw(img.double().abs(), wide.double().abs())


def head_gin(g_img, wt):
    return F.conv2d(g_img, wt, None, 2, 1)


def head_gin_bound(g_img, wt):
    return 1.01 * 48 * U * head_gin(g_img.double().abs(), wt.double().abs())


def rule2(name, got, g64, g32, hold=True):
    """The project's rule: max |got - g64| <= 4 max(E32, 1e-6 max |g64|); prints error / bound -> the ratio (hold=False: the caller
    asserts, after it has printed every figure)"""
    assert got.shape == g64.shape and torch.isfinite(got).all(), name
    E32 = (g32.double() - g64).abs().max().item()
    err, bound = (got.double().cpu() - g64).abs().max().item(), 4 * max(E32, 1e-6 * g64.abs().max().item())
    print(f"{name}: |y - g64| {err:.3e} <= {bound:.3e} ({err / bound if bound else float('nan'):.3f} of the bound; E32 {E32:.3e}, max |g64| "
          f"{g64.abs().max().item():.3e})")
    assert err <= bound or not hold, (name, err, bound)
    return err / bound if bound else float(err > 0)


def within(name, got, want, bound):
    """|got - want| <= bound elementwise (a bound of 0 asks for equality); prints the largest error / bound"""
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    err = (got.double().cpu() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, error / bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)
    return ratio


# ---- the stride-2 forms as their equivalent 3 x 3 problems -------------------------------------------------------------------------------
def _map(r, f):
    return cref.Gradient(f(r.T), f(r.S), f(r.y32), f(r.g64), r.E32)


def stride2_reference(x, w, g, relu_in, transposed):
    """x, w, g on the CPU in fp32 -> cref.Reference for conv2d(act(x), w (Co, Ci, 4, 4), stride 2, padding 1) or, transposed,
    conv_transpose2d(act(x), w (Ci, Co, 4, 4), stride 2, padding 1): T / S / y32 / g64 / E32 of the equivalent 3 x 3 problem on the
    space-to-depth operands, the weight's folded, the input's brought back to x's pixels and masked by x > 0 where the ReLU is there"""
    a = torch.relu(x) if relu_in else x
    mask = (x > 0) if relu_in else torch.ones_like(x, dtype=torch.bool)
    if not transposed:
        r = cref.reference(_s2d(a).contiguous(), s2d_weight(w), g)
        gx = _map(r.x, lambda t: _d2s(t.contiguous(memory_format=torch.channels_last), x.size(1)).contiguous() * mask.to(t.dtype))
        return cref.Reference(gx, _map(r.weight, fold), r.bias, r.s)
    r = cref.reference(a, convt_weight(w), _s2d(g).contiguous(), has_bias=False)
    d = torch.double
    Tb = g.to(d).sum((0, 2, 3))
    y32 = g.sum((0, 2, 3))
    bias = cref.Gradient(Tb, g.to(d).abs().sum((0, 2, 3)), y32, Tb, (y32.to(d) - Tb).abs().max().item())
    return cref.Reference(_map(r.x, lambda t: t * mask.to(t.dtype)), _map(r.weight, fold_t), bias, r.s)


def plain_reference(x, w, g, relu_in):
    a = torch.relu(x) if relu_in else x
    mask = (x > 0) if relu_in else torch.ones_like(x, dtype=torch.bool)
    r = cref.reference(a, w, g)
    return cref.Reference(_map(r.x, lambda t: t * mask.to(t.dtype)), r.weight, r.bias, r.s)


# ---- twins of the encoder and the decoder with given ReLU decisions -----------------------------------------------------------------------
class Masks:
    """The ReLU decisions of a run, in the order the ReLUs are met; `near` and `flipped` count, over all of them, the twin's
    pre-activations within 1e-4 max |.| of zero and the decisions that differ from the twin's own signs"""

    def __init__(self, masks):
        self.masks, self.at, self.near, self.flipped, self.total = masks, 0, 0, 0, 0

    def relu(self, t, count=True):
        m = self.masks[self.at].to(t.device)
        self.at += 1
        assert m.shape == t.shape, (self.at, tuple(m.shape), tuple(t.shape))
        if count:
            d = t.detach()
            self.near += int((d.abs() <= 1e-4 * d.abs().max()).sum())
            self.flipped += int(((d > 0) != m).sum())
            self.total += d.numel()
        return t * m.to(t.dtype)


def _res(t, block, P, mk, count):
    w3, b3, w1, b1 = (P[id(p)] for p in (block.conv[1].weight, block.conv[1].bias, block.conv[3].weight, block.conv[3].bias))
    r = mk.relu(t, count)
    return F.conv2d(mk.relu(F.conv2d(r, w3, b3, padding=1), count), w1, b1) + r


def _c(conv, P):
    return P[id(conv.weight)], P[id(conv.bias)]


def twin_params(params, dtype):
    """{id(parameter): its copy in `dtype` on the host, a leaf that requires grad}"""
    return {id(p): p.detach().cpu().to(dtype).clone().requires_grad_() for p in params}


def encoder_params(m):
    return [p for mod in (m.enc_b, m.enc_t, m.quantize_conv_t) for p in mod.parameters()]


def decoder_params(m):
    return [p for mod in (m.upsample_t, m.dec) for p in mod.parameters()]


def encoder_twin(m, P, x, mk, count=True):
    """quantize_conv_t(enc_t(enc_b(x))) on the copies P of m's parameters, the ReLU decisions those of mk"""
    eb, et = m.enc_b.blocks, m.enc_t.blocks
    h = F.conv2d(x, *_c(eb[0], P), 2, 1)
    h = F.conv2d(mk.relu(h, count), *_c(eb[2], P), 2, 1)
    h = F.conv2d(mk.relu(h, count), *_c(eb[4], P), 1, 1)
    h = _res(_res(h, eb[5], P, mk, count), eb[6], P, mk, count)
    h = F.conv2d(mk.relu(h, count), *_c(et[0], P), 2, 1)
    h = F.conv2d(mk.relu(h, count), *_c(et[2], P), 1, 1)
    h = _res(_res(h, et[3], P, mk, count), et[4], P, mk, count)
    return F.conv2d(mk.relu(h, count), *_c(m.quantize_conv_t, P))


def decoder_twin(m, P, q, mk, count=True):
    """dec(upsample_t(q)) likewise"""
    dc = m.dec.blocks
    h = F.conv_transpose2d(q, *_c(m.upsample_t, P), 2, 1)
    h = F.conv2d(h, *_c(dc[0], P), 1, 1)
    h = _res(_res(h, dc[1], P, mk, count), dc[2], P, mk, count)
    h = F.conv_transpose2d(mk.relu(h, count), *_c(dc[4], P), 2, 1)
    return F.conv_transpose2d(mk.relu(h, count), *_c(dc[6], P), 2, 1)
