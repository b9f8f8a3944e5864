"""GPU: ps_vq_nearest_f32 / ps_vq_embed_f32 (csrc/vq.hip) through the C ABI, bit for bit against the oracle's restatement of the header's
definition (oracle/pixelsynth_oracle.c: ps_oracle_vq_nearest, itself held to float64 by tests/test_vq_nearest_cpu.py), and the two
module surfaces that hand the codes on.  No assertion here has a tolerance, except the 8 codes MIOpen's near-ties get in the last test.

The geometry that matters in k_vq_nearest: 16 rows per workgroup, 256 threads striding over K (a thread's codes are k, k + 256, ...),
four waves of 64 merged by shuffles inside a wave and through LDS across them.

The calls on hostile rows only read idx back: no code from them is handed to another kernel before its range has been asserted."""
import numpy as np
import pytest
import torch

import _vq_nearest_cases as cases
from oracle import c_oracle
from pixelsynth_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
bits = cases.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nearest(z, emb, layout=0, hw=1):
    """z: (N, D) [layout 0] or (B, D, HW) [layout 1] numpy, emb (D, K) numpy -> idx (N,) int32, mindist (N,) f32 as numpy"""
    D, K = emb.shape
    n = z.size // D
    d_z, d_emb = dev(z), dev(emb)
    idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    md = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    rc = _lib.lib().ps_vq_nearest_f32(_lib.ptr(d_z), layout, _lib.ptr(d_emb), n, D, K, hw, _lib.ptr(idx), _lib.ptr(md), _lib.current_stream())
    _lib.check(rc, "ps_vq_nearest_f32")
    return idx.cpu().numpy(), md.cpu().numpy()


def assert_same(got, want):
    """(idx, mindist) pairs: the codes equal, the distances equal as bit patterns"""
    assert np.array_equal(got[0], want[0]), f"{(got[0] != want[0]).sum()} codes differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{(bits(got[1]) != bits(want[1])).sum()} distances differ in their bits"


@pytest.mark.parametrize("N,D,K", [s for s in cases.SHAPES if s[0] != 1000] + [(16, 64, 512), (48, 64, 255)])
def test_layout_0_is_the_oracle_bit_for_bit(N, D, K):
    z, emb = cases.random_case(N, D, K)
    assert_same(nearest(z, emb), c_oracle.vq_nearest(z, emb))


def test_exact_ties_take_the_smaller_index():
    """cases.TIE_PAIRS says which pair meets where: inside one wave (3, 5), across waves (10, 70), in one thread's scan (100, 356), with
    the smaller k in the higher wave (255, 256) and (511, 512), first against last column (0, 699)."""
    z, emb, want = cases.tie_case()
    idx, md = nearest(z, emb)
    assert np.array_equal(idx, want)
    assert np.array_equal(bits(md), np.zeros(len(want), np.int32))
    assert_same((idx, md), c_oracle.vq_nearest(z, emb))
    z, emb = cases.identical_columns_case()
    got = nearest(z, emb)
    assert np.array_equal(got[0], np.zeros(len(z), np.int32))       # 700 equal distances per row, over every merge at once
    assert_same(got, c_oracle.vq_nearest(z, emb))


@pytest.mark.parametrize("B,D,HW,K", [(3, 64, 40, 512), (2, 5, 7, 37), (1, 64, 1024, 512)])
def test_layout_1_is_layout_0_on_the_permuted_copy(B, D, HW, K):
    """HW = 40 and 7 are no multiple of 16: a 16-row workgroup straddles two images (n / HW changes inside it)."""
    z, emb = cases.random_case(B * HW, D, K)
    flat = nearest(z, emb)
    assert_same(nearest(cases.to_layout1(z, B, HW), emb, 1, HW), flat)
    assert_same(flat, c_oracle.vq_nearest(z, emb))


@pytest.mark.parametrize("layout", [0, 1])
def test_hostile_rows_give_code_0_and_leave_their_neighbours_alone(layout):
    z, clean, emb = cases.hostile_case()
    K, bad = emb.shape[1], list(cases.HOSTILE_ROWS)
    shape = (lambda a: a) if layout == 0 else (lambda a: cases.to_layout1(a, 3, 16))
    hw = 1 if layout == 0 else 16
    idx, md = nearest(shape(z), emb, layout, hw)
    assert idx.min() >= 0 and idx.max() < K, f"codes outside [0, {K}): {idx[(idx < 0) | (idx >= K)]}"
    assert np.array_equal(idx[bad], np.zeros(len(bad), np.int32))
    assert np.all(np.isposinf(md[bad]))
    assert_same((idx, md), c_oracle.vq_nearest(z, emb))
    good = np.setdiff1d(np.arange(len(z)), bad)
    idx0, md0 = nearest(shape(clean), emb, layout, hw)
    assert np.array_equal(idx[good], idx0[good]) and np.array_equal(bits(md[good]), bits(md0[good]))


def test_codebook_columns_that_are_not_finite_are_never_chosen():
    z, emb = cases.hostile_codebook_case()
    got = nearest(z, emb)
    assert got[0].min() >= 0 and got[0].max() < emb.shape[1]
    assert not np.isin(got[0], cases.BAD_COLUMNS).any()
    assert_same(got, c_oracle.vq_nearest(z, emb))


@pytest.mark.parametrize("B,D,HW,K", [(3, 5, 7, 37), (2, 64, 40, 512)])
def test_embed_gather_is_numpys_with_zeros_at_invalid_codes(B, D, HW, K):
    """B * D * HW = 105: less than one 256-thread workgroup, so its tail threads must stay out; 5120: twenty workgroups, b, d and p all
    change inside one.  HW is no multiple of 16 or 64 in either."""
    rs = np.random.RandomState(B + D + HW + K)
    emb = rs.randn(D, K).astype(np.float32)
    codes = rs.randint(0, K, (B, HW)).astype(np.int32)
    codes[0, 0], codes[0, HW - 1] = 0, K - 1
    invalid = [(-1, (0, 1)), (K, (0, 2)), (np.iinfo(np.int32).max, (B - 1, HW - 2)), (np.iinfo(np.int32).min, (B - 1, 3))]
    for v, at in invalid:
        codes[at] = v
    d_codes, d_emb = dev(codes), dev(emb)
    out = torch.full((B, D, HW), float("nan"), device="cuda")
    rc = _lib.lib().ps_vq_embed_f32(_lib.ptr(d_codes), _lib.ptr(d_emb), B, HW, D, K, _lib.ptr(out), _lib.current_stream())
    _lib.check(rc, "ps_vq_embed_f32")
    valid = (codes >= 0) & (codes < K)
    want = emb[:, np.where(valid, codes, 0)].transpose(1, 0, 2)                          # (B, D, HW)
    want = np.where(valid[:, None, :], want, np.float32(0.0)).astype(np.float32)
    assert (~valid).sum() == 4
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_refusals():
    L = _lib.lib()
    z, emb = dev(np.zeros((48, 64), np.float32)), dev(np.zeros((64, 512), np.float32))
    idx = torch.full((48,), -7, dtype=torch.int32, device="cuda")

    def refused(layout, N, D, K, HW):
        rc = L.ps_vq_nearest_f32(_lib.ptr(z), layout, _lib.ptr(emb), N, D, K, HW, _lib.ptr(idx), None, _lib.current_stream())
        msg = L.ps_last_error()
        return rc != 0 and bool(msg) and b"vq_nearest" in msg

    assert refused(1, 48, 64, 512, 7)        # layout 1: N is no multiple of HW
    assert refused(1, 48, 64, 512, 0)
    assert refused(2, 48, 64, 512, 1)        # no such layout
    assert refused(0, 48, 64, 0, 1)          # K = 0
    assert refused(0, 48, 0, 512, 1)         # D = 0
    torch.cuda.synchronize()
    assert bool((idx == -7).all())           # nothing was launched


def test_quantize_eval_keeps_a_nan_row_in_range():
    """Quantize.forward in eval mode hands the codes to F.embedding, which does not guard: nearest() first, its range asserted, and only
    then forward."""
    from pixelsynth_amd.vqvae2.vqvae import Quantize
    torch.manual_seed(3)
    q = Quantize(64, 512).eval().cuda()
    x = torch.randn(48, 64, device="cuda")
    x[21, 9] = float("nan")
    codes = q.nearest(x, 0).cpu().numpy()
    assert codes.dtype == np.int32 and codes.min() >= 0 and codes.max() < 512, codes[(codes < 0) | (codes >= 512)]
    assert codes[21] == 0
    want, _ = c_oracle.vq_nearest(x.cpu().numpy(), q.embed.cpu().numpy())
    assert np.array_equal(codes, want)
    with torch.no_grad():
        quantize, _diff, ind = q(x)
    assert np.array_equal(ind.cpu().numpy(), want.astype(np.int64))
    assert torch.equal(quantize, q.embed.t()[ind])


def test_encode_codes_keeps_a_nan_pixel_in_range():
    """One NaN pixel: the split-fp16 guard fires, encode_codes runs again in fp32 through torch, the latent around the pixel is NaN and
    layout 1 of the kernel quantises it.  The codes are 0 where the same module on the host (fp32) has a latent that is not finite;
    elsewhere they are the clean image's fp32-path codes, up to the 8 near-ties that
    test_encoder_runs_again_in_fp32_when_an_activation_leaves_fp16s_range (tests/test_vqvae_gpu.py) allows MIOpen."""
    from pixelsynth_amd.networks import architectures as A
    from pixelsynth_amd.vqvae2 import VQVAETop
    sd = {k: torch.from_numpy(v) for k, v in syn.vqvae_state_dict(2).items()}
    host = VQVAETop().eval()
    host.load_state_dict(sd, strict=True)
    m = VQVAETop().eval()
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    clean = torch.from_numpy(syn.image(5, 1, 3, 256))
    img = clean.clone()
    img[0, 0, 0, 0] = float("nan")
    with torch.no_grad():
        lat = host.quantize_conv_t(host.enc_t(host.enc_b(img)))              # (1, 64, 32, 32)
        hit = ~torch.isfinite(lat).all(1).reshape(-1).numpy()
        assert 0 < hit.sum() < hit.size
        with pytest.warns(UserWarning, match="run again in fp32"):
            got = m.encode_codes(img.cuda())
        assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (1, 32, 32)
        got = got.cpu().numpy().reshape(-1)
        assert got.min() >= 0 and got.max() < 512, got[(got < 0) | (got >= 512)]
        assert np.all(got[hit] == 0)
        with A.decoder_conv("fp32"):
            want = m.encode_codes(clean.cuda()).cpu().numpy().reshape(-1)
        assert (got[~hit] != want[~hit]).sum() <= 8
    A.check_f16x3_overflow(torch.device("cuda", torch.cuda.current_device()))          # (left clear)
