"""CPU: the host split the split-fp16 tests build their reference from (tests/_conv_f16x3_ref.split: hi = fp16(v), lo = fp16(v - hi),
the kernel's stash() and k_pack restated) over the whole documented range.  csrc/conv_f16x3.hip's header: 22 of fp32's 24 mantissa
bits; below 2^-3 the low half is subnormal and the split is exact to 2^-25 absolute.  So for |v| <= 65000
    |v - hi - lo| <= max(2^-22 |v|, 2^-25).
(hi is v to 11 bits, |v - hi| <= 2^-11 |v|, exact in fp32; lo is that to 11 bits again while it is a normal fp16, |lo| >= 2^-14, and to
half of fp16's subnormal spacing 2^-24 below.)"""
import numpy as np
import pytest
import torch

import _conv_f16x3_ref as M


@pytest.mark.parametrize("k", [15, 0, -3, -6, -10, -14, -18, -24, -30])
def test_host_split_keeps_22_bits_or_2_to_the_minus_25(k):
    g = torch.Generator().manual_seed(100 + k)
    v = torch.randn(2_000_000, generator=g) * 2.0 ** k
    v = v[v.abs() <= 65000.0]
    assert v.numel() > 1_000_000                      # (k = 15: |randn| <= 1.98, nineteen in twenty)
    hi, lo = M.split(v)
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    err = (v.double() - hi.double() - lo.double()).abs()
    bound = torch.clamp_min(v.double().abs() * 2.0 ** -22, 2.0 ** -25)
    worst = (err / bound).max().item()
    print(f"2^{k}: max |v - hi - lo| / max(2^-22 |v|, 2^-25) = {worst:.3f}")
    assert worst <= 1.0
    # the halves are fp16 values, and the first is the nearest one
    assert torch.equal(hi, hi.half().float()) and torch.equal(lo, lo.half().float())
    assert ((v - hi).abs().double() <= v.double().abs() * 2.0 ** -11 + 2.0 ** -25).all()


def test_host_split_at_the_edges_by_hand():
    """65000 = 2^15 * 1.98...: fp16 spacing 32 there, hi = 64992, lo = 8; 2^-3 + 2^-14 + 2^-25 is just beyond the middle of
    fp16's spacing 2^-13 there: hi = 2^-3 + 2^-13, and v - hi = -(2^-14 - 2^-25) lies in the subnormal range (spacing 2^-24), a tie that
    goes to the even neighbour -2^-14: what is left is 2^-25, the documented absolute bound, attained; a value below half of fp16's
    smallest subnormal splits to zero."""
    v = torch.tensor([65000.0, -65000.0, 2.0 ** -3 + 2.0 ** -14 + 2.0 ** -25, 2.0 ** -26, 0.0, 1.0 + 2.0 ** -11 + 2.0 ** -22])
    hi, lo = M.split(v)
    assert hi.tolist() == [64992.0, -64992.0, 2.0 ** -3 + 2.0 ** -13, 0.0, 0.0, 1.0 + 2.0 ** -10]
    np.testing.assert_array_equal(lo.numpy()[:5], np.float32([8.0, -8.0, -2.0 ** -14, 0.0, 0.0]))
    assert (v[2].double() - hi[2].double() - lo[2].double()).item() == 2.0 ** -25
    assert lo[5].item() == -(2.0 ** -11) + 2.0 ** -22       # (eleven bits of the low half as well: 1 + 2^-11 + 2^-22 splits exactly)
