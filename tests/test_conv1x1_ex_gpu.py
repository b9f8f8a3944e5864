"""GPU: ps_conv1x1_ex_nhwc_f32 (csrc/conv1x1.hip) through the C ABI -- the 1 x 1 convolution with everything the VQ-VAE fast path asks of
it: rows `ldx` floats apart of which the first Ci are read, ReLU on the way in, bias and the other branch (ReLU'd or not) on the way out.

Two assertions per call:
  * against fp64 on the host, act(x[:, :Ci]) @ w.T + bias + act_res(res): within 2e-6 of the fp64 result's largest magnitude (the
    kernel's contract in tests/test_networks_gpu.py; operands of order 1, so the output stays of the convolution's order);
  * bit for bit against the composition: ps_conv1x1_nhwc_f32 on a contiguous relu?(x[:, :Ci]), then + bias, then + relu?(res) in torch
    fp32.  The epilogue is (acc + bias) + relu?(res) in plain fp32 adds -- nothing in it can contract -- so the vector stores (Co a
    multiple of 4) and the scalar ones must give exactly that.
x[:, Ci:] is NaN (never read into a product), y a NaN-filled, 16-byte aligned view inside a larger buffer whose ends hold a sentinel.

Measured on the MI355X (printed by the tests): MEASURED_MAXIMA below."""
import copy

import pytest
import torch

from pixelsynth_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED_MAXIMA = """
largest error against fp64, of the result's largest magnitude (bound 2e-6), over npix x ldx x flags x bias x res:
  Ci =   4: 1.2e-7     Ci =  32: 2.7e-7     Ci =  64: 3.9e-7     Ci = 128: 6.1e-7 (128 -> 256: 5.0e-7)     Ci = 256: 7.3e-7
  second trip of the persistent loop: 4 -> 16 7.7e-8, 128 -> 128 2.7e-7, 256 -> 128 2.8e-7
_FastPath.res: err 4.4e-7, err32 1.3e-7, ratio 3.26 (K = 10)
"""

BOUND = 2e-6
K_BLOCK = 10.0     # the block-level bound of tests/test_block_routes_gpu.py
SENTINEL = -777.0
GUARD = 4            # floats in front of y: y starts 16 bytes into its buffer


def _data(npix, Ci, Co, ldx, seed):
    """x (npix, ldx) with NaN beyond Ci, w (Co, Ci), bias (Co), res (npix, Co) on the host: about half of x and res negative."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((npix, ldx), float("nan"))
    x[:, :Ci] = torch.randn(npix, Ci, generator=g)
    return x, torch.randn(Co, Ci, generator=g) / Ci ** 0.5, torch.randn(Co, generator=g), torch.randn(npix, Co, generator=g)


def _ex(x, ldx, w, bias, res, flags, npix, Ci, Co):
    """One call; -> y (npix, Co), checked: the sentinels either side of it untouched, no NaN left in it."""
    buf = torch.full((GUARD + npix * Co + 64,), SENTINEL, device=DEV)
    y = buf[GUARD:GUARD + npix * Co]
    y.fill_(float("nan"))
    assert y.data_ptr() % 16 == 0
    p = lambda t: None if t is None else t.data_ptr()
    rc = _lib.lib().ps_conv1x1_ex_nhwc_f32(x.data_ptr(), ldx, w.data_ptr(), p(bias), p(res), flags, npix, Ci, Co, y.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ps_conv1x1_ex_nhwc_f32")
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + npix * Co:] == SENTINEL).all()), "wrote outside y"
    assert not bool(torch.isnan(y).any()), "a pixel was not written, or NaN beyond Ci reached a product"
    return y.view(npix, Co)


def _plain(xc, w, npix, Ci, Co):
    """ps_conv1x1_nhwc_f32 on a contiguous (npix, Ci) x: the entry point tests/test_networks_gpu.py pins against fp64."""
    y = torch.full((npix, Co), float("nan"), device=DEV)
    _lib.check(_lib.lib().ps_conv1x1_nhwc_f32(xc.data_ptr(), w.data_ptr(), npix, Ci, Co, y.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "ps_conv1x1_nhwc_f32")
    return y


def _refs(x, w, bias, res, Ci, combos):
    """The fp64 result of every combination, and the smallest share its largest magnitude has of its largest term's."""
    x64, w64 = x[:, :Ci].double(), w.double()
    conv = {0: x64 @ w64.t(), 1: torch.relu(x64) @ w64.t()}
    refs, share = [], 1.0
    for flags, use_bias, use_res in combos:
        terms = [conv[flags & 1]] + ([bias.double().expand_as(conv[0])] if use_bias else []) + (
            [(torch.relu(res) if flags & 2 else res).double()] if use_res else [])
        ref = sum(terms[1:], terms[0])
        refs.append(ref)
        share = min(share, ref.abs().max().item() / max(1e-30, *(t.abs().max().item() for t in terms)))      # (a ReLU'd term may be all zero)
    return refs, share


def _check(npix, Ci, Co, ldx, seed, combos):
    """Every (flags, bias?, res?) of `combos` on one set of operands; -> the largest error against fp64, as a share of the bound's scale.
    The bound is a share of the RESULT's largest magnitude and presumes that this is of the convolution's order: 1, the standard
    deviation of a product of these operands (0.7 behind the ReLU).  An output of one or three numbers need not be: 128 products that
    sum to -0.17 plus a bias of 0.12 leave 0.05, and the exact fp32 sum -- 1.7e-7 off, 2e-8 of the products' magnitudes -- is then 3e-6
    of the result.  So operands whose fp64 result, in any combination, has a largest magnitude below 0.5, or below a quarter of its
    largest term, are drawn again: a rule on the reference alone, which leaves the bound at 1e-6 absolute or more, where fp32's own
    error over 256 products (up to 4e-7 here) still fits."""
    for draw in range(64):
        x, w, bias, res = _data(npix, Ci, Co, ldx, seed + 7919 * draw)
        refs, share = _refs(x, w, bias, res, Ci, combos)
        if share >= 0.25 and min(r.abs().max().item() for r in refs) >= 0.5:
            break
    else:
        raise AssertionError("no operands of the convolution's order in 64 draws")
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), bias.to(DEV), res.to(DEV)
    xc = xd[:, :Ci].contiguous()
    conv32 = {0: _plain(xc, wd, npix, Ci, Co), 1: _plain(torch.relu(xc), wd, npix, Ci, Co)}
    worst = 0.0
    for (flags, use_bias, use_res), ref in zip(combos, refs):
        tag = f"npix {npix} Ci {Ci} Co {Co} ldx {ldx} flags {flags} bias {use_bias} res {use_res}"
        got = _ex(xd, ldx, wd, bd if use_bias else None, rd if use_res else None, flags, npix, Ci, Co)
        want = conv32[flags & 1]
        if use_bias:
            want = want + bd
        if use_res:
            want = want + (torch.relu(rd) if flags & 2 else rd)
        assert torch.equal(got, want), tag + ": not the composition, bit for bit"
        err = (got.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        assert err <= BOUND, (tag, err)
        worst = max(worst, err)
    return worst


ALL = [(f, b, r) for f in range(4) for b in (False, True) for r in (False, True)]
NPIX = [1, 15, 17, 255, 256, 257, 3 * 256 + 37]      # less than a tile; a clamped last pixel; an idle wave; a partial last trip
# Co: 1, 3, 6 scalar stores; 20, 36 vector stores with a last tile that is partly (co >= Co) empty; 64, 128 full tiles; Ci x 128 = 64 KB / 128 KB
# of weights: two / one workgroup per compute unit; 128 -> 256 (the decoder's widest projection) fills the 128 KB too
CI_CO = [(Ci, Co) for Ci in (4, 32, 64, 128, 256) for Co in (1, 3, 6, 20, 36, 64, 128)] + [(128, 256)]


@pytest.mark.parametrize("Ci,Co", CI_CO)
def test_conv1x1_ex_against_fp64_and_bit_for_bit_against_its_composition(Ci, Co):
    """Every instantiation (Ci = 4, 32, 64, 128, 256) x Co x npix x ldx in {Ci, Ci + 4, 2 Ci} x flags 0-3 x bias x res."""
    assert _lib.lib().ps_conv1x1_takes(Ci, Co) == 1
    worst = 0.0
    for npix in NPIX:
        for ldx in sorted({Ci, Ci + 4, 2 * Ci}):
            worst = max(worst, _check(npix, Ci, Co, ldx, 1000 * Ci + 10 * Co + npix % 7, ALL))
    print(f"conv1x1_ex {Ci} -> {Co}: worst error {worst:.3e} of the output's largest magnitude (bound {BOUND:.0e})")


@pytest.mark.parametrize("Ci,Co,per_cu", [(4, 16, 4), (128, 128, 2), (256, 128, 1)])
def test_conv1x1_ex_persistent_loop_takes_its_second_trip(Ci, Co, per_cu):
    """cus * per_cu workgroups of 256 pixels each (per_cu by the LDS the weights take: 1 KB, 64 KB, 128 KB): 37 pixels more than they cover
    in one trip, so workgroup 0 goes round again for a partial tile; ReLU in, bias, ReLU'd res."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    npix = 256 * cus * per_cu + 37
    worst = _check(npix, Ci, Co, Ci, Ci + Co, [(3, True, True)])
    print(f"conv1x1_ex {Ci} -> {Co}, {npix} pixels: worst error {worst:.3e}")


def test_conv1x1_ex_refuses_what_it_does_not_take():
    """Return code and ps_last_error() for each rule of the entry point; nothing is launched.  What does not fit is 256 -> 256; 128 -> 256 and
    256 -> 128 both fill the 128 KB exactly and are taken (the decoder's 128 -> 256 Down block projects through the former)."""
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    Ci, Co, npix = 32, 64, 48
    x, w, bias, res = (t.to(DEV) for t in _data(npix, Ci, Co, 2 * Ci, 1))
    y = torch.full((npix, Co), SENTINEL, device=DEV)
    spare_b, spare_r = torch.zeros(Co + 4, device=DEV), torch.zeros(npix * Co + 4, device=DEV)

    def refused(text, ldx=2 * Ci, b=bias.data_ptr(), r=res.data_ptr(), flags=3, n=npix, ci=Ci, co=Co):
        rc = L.ps_conv1x1_ex_nhwc_f32(x.data_ptr(), ldx, w.data_ptr(), b, r, flags, n, ci, co, y.data_ptr(), st)
        assert rc != 0 and text in L.ps_last_error(), (text, rc, L.ps_last_error())
    refused(b"ldx >= Ci", ldx=Ci - 4)
    refused(b"multiple of 4 required (ldx = 34)", ldx=Ci + 2)
    refused(b"unknown flags 4", flags=4)
    refused(b"16-byte aligned", b=spare_b.data_ptr() + 4)
    refused(b"16-byte aligned", r=spare_r.data_ptr() + 4)
    refused(b"no pixels", n=0)
    refused(b"ceil16(Co) * Ci <= 32768", ci=256, co=256)         # 256 KB of weights: more than a workgroup can keep
    refused(b"Ci in {4, 32, 64, 128, 256}", ci=48)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert L.ps_conv1x1_takes(256, 256) == 0 and L.ps_conv1x1_takes(128, 256) == 1 and L.ps_conv1x1_takes(256, 128) == 1


def test_vqvae_fast_path_res_block_against_the_module_in_fp64():
    """_FastPath.res alone (vqvae2/vqvae.py): conv1x1(relu(conv3x3(relu(x)))) + relu(x) as one split-fp16 launch and one
    ps_conv1x1_ex_nhwc_f32 launch (ldx = 64 > Ci = 32, flags 3, bias, res = x) against the module's ResBlock in fp64 on the host.  The
    skip branch sees relu(x), so x has negative entries.  Bound: K * err32 of tests/test_block_routes_gpu.py -- err32 the error of the
    ResBlock's own fp32 forward on the host against the same fp64 output, K = 10."""
    from pixelsynth_amd.networks.f16x3 import check_f16x3_overflow
    from pixelsynth_amd.vqvae2.vqvae import VQVAETop
    m = VQVAETop().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.vqvae_state_dict(0).items()}, strict=True)
    block = m.enc_b.blocks[5]
    x = torch.randn(2, 128, 16, 16, generator=torch.Generator().manual_seed(9))
    assert (x < 0).float().mean() > 0.4
    with torch.no_grad():
        ref = copy.deepcopy(block).double()(x.double())
        top = ref.abs().max().item()
        err32 = (block(x).double() - ref).abs().max().item() / top
        m = m.to(DEV)
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
        fast = m._fast(xd, 256, 256)
        assert fast is not None
        got = fast.res(xd, fast.eb_res[0])
        check_f16x3_overflow(xd.device)
    err = (got.cpu().double() - ref).abs().max().item() / top
    print(f"_FastPath.res: err {err:.3e} err32 {err32:.3e} ratio {err / err32:.2f}")
    assert got.shape == ref.shape and 2e-8 < err32 < 1e-6
    assert err <= K_BLOCK * err32, (err, err32, err / err32)
