"""GPU: csrc/conv_f16x3.hip at the two ends of the split's range.  The older tests feed x ~ 1.5 randn and look at one number per tensor,
max |y - ref| / max |ref|: an error confined to small outputs, or to small INPUTS, is invisible to them.  Here the activated values sit
at 2^k, k from -20 (every low half a subnormal fp16 or zero: the split keeps 2^-25 ABSOLUTE, not 22 bits) to 2^14 clipped at 6.4e4 (the
low half carries up to 16), the weights at their usual scale and at 2^-12 of it, and the measure is per element (tests/_conv_f16x3_ref.py):
T holds the split's representation error already, so r16 <= 10 r32 isolates the kernel -- does it multiply subnormal halves, does a
large high half swamp the sums.

What the split itself loses is held to the documented model, not to a tolerance: with ex = xa - xh - xl, ew = w - wh - wl,
    conv64(xa, w) - T = conv(xl, wl) + conv(ex, w) + conv(xa, ew) - conv(ex, ew)
so  |conv64(xa, w) - T| <= conv(|xl|, |wl|) + conv(|ex|, |w|) + conv(|xa|, |ew|) + conv(|ex|, |ew|)   element by element; the first term
is the product the kernel drops by design ("below 2^-22 relative" in its header), the others are the per-element residuals.

The shape is the walk tests' fused case (Co = 128, Ci = 64, 64 x 64, the smallest batch with three items per workgroup, a scale / shift
per frame).  Every case prints r16, r32, max |T - conv64| / max |conv64| and the worst |T - conv64| / model before it asserts.
"""
import pytest
import torch

import _conv_f16x3_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("wk", [0, -12])
@pytest.mark.parametrize("k", [-20, -12, -6, 0, 10, 14])
def test_split_fp16_convolution_from_subnormal_halves_to_the_top_of_fp16(k, wk):
    """Activations 2^k |randn|-sized (x = 2^k randn, scale in [0.5, 1), shift = 2^k * 0.3 randn, so that the ACTIVATED value is at that
    scale), x clipped to +-6.2e4 (bites at k = 14: activated values up to 6.4e4, under the guard's 65000); weights 2^wk / (3 sqrt(Ci))."""
    H = W = 64
    Ci, Co = 64, 128
    B, p = M.smallest_batch(lambda p: p["longest"] >= 3 and p["frame_changes"] > 0, H, W, Co)
    g = torch.Generator().manual_seed(200 + k - wk)
    x = (torch.randn(B, Ci, H, W, generator=g) * 2.0 ** k).clamp_(-6.2e4, 6.2e4).to(DEV)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) * 2.0 ** wk / (3 * Ci ** 0.5)).to(DEV)
    sc = (torch.rand(B, Ci, generator=g) * 0.5 + 0.5).to(DEV)
    sh = (torch.randn(B, Ci, generator=g) * 0.3 * 2.0 ** k).clamp_(-1.5e3, 1.5e3).to(DEV)
    xa = M.activated(x, sc, sh)
    top = xa.max().item()
    assert top <= 6.4e4 and (k < 14 or top > 6.0e4)
    r = M.reference(xa, w)
    y, flag = M.run(x, M.pack(w), Co, sc, sh)
    assert int(flag.item()) == 0
    # the representation error of the split against its documented model
    (xh, xl), (wh, wl) = M.split(xa), M.split(w)
    ex, ew = (xa.double() - xh.double() - xl.double()).abs(), (w.double() - wh.double() - wl.double()).abs()
    model = M.conv64(xl.abs(), wl.abs()) + M.conv64(ex, w.abs()) + M.conv64(xa.abs(), ew) + M.conv64(ex, ew)
    gap = (r.ref - r.T).abs()
    print(f"x 2^{k} w 2^{wk}: B {B} top {top:.4g}; max |T - conv64| / max |conv64| = {gap.max().item() / r.ref.abs().max().item():.3e}, "
          f"max over elements of |T - conv64| / model = {(gap / model.clamp_min(1e-300)).max().item():.3f}")
    assert (gap <= model * (1 + 1e-9) + 1e-300).all()
    M.hold(y, r, f"x 2^{k} w 2^{wk}", end_to_end=k >= 0 and wk == 0)
