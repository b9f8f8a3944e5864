"""GPU: ps_fid_conv, ps_fid_pool and ps_fid_input (csrc/fid.hip) off the shapes Inception-v3 happens to have.

Exact, no tolerance: every case of tests/_fid_edge_cases.py on integer-valued operands (any summation order is exact) against
relu(conv2d) in fp64 on the CPU, into a fresh map and at two channel offsets of a wider map whose other channels keep their bits, with
NaN behind the channels of x the layer reads.  Order: on operands that make every output the same sum, all N Ho Wo x Co outputs are one
bit pattern; a batch, a split of it and a single image give the same bits per image.  Rounding at the stage boundaries (K = 256, 320,
1024, 1040) and the averaging pools: the largest error against fp64 at most 4 x that of torch's own fp32 operator on the same operands,
measured in the same test (the bound of tests/test_fid_gpu.py).  The refusals of ps_fid_conv leave the output untouched.  The pools on
maps of 1 x 1 to 5 x 4, with ldx > C and a channel offset.  The input pass on sources from 1 x 1 to 1000 x 37 against a float32
restatement of the kernel's formula bit for bit, against torch's CPU bilinear resize (bit for bit where EXACT_AS_TORCH says so, the
4 x bound elsewhere), at its corners, and on strided and uint8 views.

Measured on the MI355X: MEASURED below."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fid_edge_cases as E
from pixelsynth_amd import _lib, fid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -1234.5
MEASURED = """one run on the MI355X:
rounding, kernel / torch fp32 (ratio): K = 256 1.106e-06 / 4.090e-06 (0.27), K = 320 9.493e-07 / 2.636e-06 (0.36), K = 1024 6.254e-07 / 1.163e-06 (0.54),
K = 1040 6.997e-07 / 4.255e-06 (0.16)
same patch: 24300, 21000, 18900 and 30000 outputs, one bit pattern each
pools on 1x1 .. 5x4: AVG_S1 kernel = torch fp32 on every map (largest 1.391e-07), MEAN kernel 0 .. 5.960e-08 against torch's 0 .. 1.623e-07
input against torch's fp32 resize on the CPU, largest difference (in ulps of a value in [0.5, 1)): 1x1 1.192e-07 (2), 2x3 3.576e-07 (6), 598x598 0,
300x298 7.391e-06 (124), 1000x37 3.576e-06 (60); against fp64, kernel / torch: 5.960e-08 / 1.192e-07, 4.111e-07 / 3.112e-07, 1.183e-07 / 1.183e-07,
6.213e-05 / 6.213e-05, 1.170e-04 / 1.170e-04.  The float32 restatement (input_mirror) holds bit for bit on all five."""


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return a.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def pack(w, b, case):
    torch.cuda.set_device(DEV)
    layer = fid.pack_conv(t(w), t(b), case[2], (case[3], case[4]))
    assert layer is not None and layer["Ci"] == case[5], case
    return layer


def ceil4(n):
    return (n + 3) // 4 * 4


def conv_fresh(x, layer):
    """fid.conv into a map of its own -> (N, Ho, Wo, Co).  ps_fid_conv takes a map whose width is a multiple of 4 (fid.conv without
    `out` makes one of Co channels, which the library refuses for any other Co): where Co is no such multiple the map has
    ceil4(Co) channels, and the one to three behind Co must keep the sentinel."""
    Co = layer["Co"]
    if Co % 4 == 0:
        return fid.conv(x, layer)
    out = torch.full((x.size(0),) + fid.conv_shape(layer, x.size(1), x.size(2)) + (ceil4(Co),), SENTINEL, device=x.device)
    fid.conv(x, layer, out, 0)
    assert bool((out[..., Co:] == SENTINEL).all()), "the channels behind Co"
    return out[..., :Co]


# ---- exact
@pytest.mark.parametrize("k", range(len(E.CASES)), ids=[E.name(c) for c in E.CASES])
def test_exact_on_integer_operands(k):
    case = E.CASES[k]
    Ci, ldx, Co, N = case[5:9]
    Ho, Wo = E.out_shape(case)
    x, w, b = E.integer_operands(k)
    want = E.reference(x, w, b, case)
    layer = pack(w, b, case)
    got = conv_fresh(t(E.widen(x, ldx)), layer)                     # NaN in the channels of x behind Ci
    assert tuple(got.shape) == (N, Ho, Wo, Co)
    assert torch.equal(got.cpu().double(), want), "a fresh map"
    if ldx > Ci:
        assert same_bits(conv_fresh(t(x), layer), got), "ldx > Ci gives the bits of ldx = Ci"
    # at a channel offset of a wider map: right behind Co (inside its last quad where Co is no multiple of 4) and further on
    for coff, ldy in ((4, 4 + ceil4(Co) + 4), (24, 24 + ceil4(Co))):
        out = torch.full((N, Ho, Wo, ldy), SENTINEL, device=DEV)
        before = out.clone()
        fid.conv(t(E.widen(x, ldx)), layer, out, coff)
        assert same_bits(out[..., coff:coff + Co], got), (coff, ldy)
        assert same_bits(out[..., :coff], before[..., :coff]) and same_bits(out[..., coff + Co:], before[..., coff + Co:]), (coff, ldy)


# ---- the order depends on nothing but the layer
@pytest.mark.parametrize("k", range(len(E.SAME_PATCH)), ids=[E.name(c) for c in E.SAME_PATCH])
def test_every_output_of_one_patch_is_one_bit_pattern(k):
    case = E.SAME_PATCH[k]
    x, w, b, value = E.same_patch_operands(case, 300 + k)
    got = conv_fresh(t(x), pack(w, b, case))
    assert tuple(got.shape) == (case[8],) + E.out_shape(case) + (case[7],)
    patterns = torch.unique(bits(got))
    first = float(got.flatten()[0])
    print(f"same patch {E.name(case)}: {got.numel()} outputs, {patterns.numel()} bit pattern(s), value {first!r} (fp64 {value!r})")
    assert first > 0 and abs(first - value) <= 1e-4 * value
    assert patterns.numel() == 1, "lanes, waves, pixel tiles, Co tiles, Co blocks and the scalar tail sum in one order"


SPLIT_CASES = [7, 8, 10, 13, 14, 22]


@pytest.mark.parametrize("k", SPLIT_CASES, ids=[E.name(E.CASES[k]) for k in SPLIT_CASES])
def test_batch_split_and_single_image_give_the_same_bits(k):
    case = E.CASES[k]
    x, w, b = E.randn_operands(case, 500 + k, N=3)
    layer, x = pack(w, b, case), t(x)
    whole = conv_fresh(x, layer)
    assert float((whole > 0).float().mean()) > 0.25
    assert same_bits(conv_fresh(x, layer), whole), "run to run"
    for lo, hi in ((0, 1), (1, 3), (2, 3), (1, 2)):
        assert same_bits(conv_fresh(x[lo:hi].contiguous(), layer), whole[lo:hi]), (lo, hi)


# ---- rounding at the stage boundaries
def test_rounding_at_the_stage_boundaries():
    torch.cuda.set_device(DEV)
    failed = []
    for k, case in enumerate(E.ROUNDING):
        _, _, s, ph, pw = case[:5]
        x, w, b = E.randn_operands(case, 700 + k)
        want = E.reference(x, w, b, case)
        got = conv_fresh(t(x), pack(w, b, case)).cpu().double()
        lib = torch.relu(F.conv2d(t(x).permute(0, 3, 1, 2), t(w), t(b), s, (ph, pw))).permute(0, 2, 3, 1).cpu().double()
        err, ref = float((got - want).abs().max()), float((lib - want).abs().max())
        print(f"rounding K = {E.K_of(case):4d} (S = {E.stages(case):2d}): kernel {err:.3e}  torch fp32 {ref:.3e}  ratio {err / ref:.2f}")
        if not err <= 4 * ref:
            failed.append((E.K_of(case), err, ref))
    assert not failed, failed


# ---- refusals
def test_refusals_leave_the_output_untouched():
    torch.cuda.set_device(DEV)
    x = torch.ones(1, 8, 8, 8, device=DEV)
    layer = fid.pack_conv(torch.ones(16, 8, 3, 3, device=DEV), torch.ones(16, device=DEV), 1, (1, 1))
    odd = torch.ones(8 * 8 * 16 + 4, device=DEV)          # odd[1:] holds either map, 4 bytes off a 16-byte boundary
    out = torch.full((1, 8, 8, 16), SENTINEL, device=DEV)

    def call(x=x, ldx=8, H=8, W=8, Ci=8, KH=3, KW=3, stride=1, ph=1, pw=1, y=out):
        _lib.call("ps_fid_conv", x, ldx, layer["wp"], layer["wp"].numel(), layer["bias"], 1, H, W, Ci, KH, KW, stride, ph, pw, 16, y, 16, 0)

    refusals = [
        (dict(KH=8), "1 <= KH, KW <= 7"), (dict(stride=3), "stride 1 or 2"), (dict(ph=3), "0 <= pad < kernel"),
        (dict(Ci=6), "Ci a multiple of 4"), (dict(ldx=4), "ldx >= Ci"), (dict(ldx=10), "ldx >= Ci and a multiple of 4"),
        (dict(H=2, ph=0), "fid_conv: N = 1, H = 2"), (dict(W=1, pw=0), "fid_conv: N = 1, H = 8, W = 1"),
        (dict(x=odd[1:]), "16-byte aligned"), (dict(y=odd[1:]), "16-byte aligned"),
    ]
    for change, why in refusals:
        with pytest.raises(RuntimeError, match="ps_fid_conv failed.*" + why):
            call(**change)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((odd == 1).all()), "nothing was launched"
    call()
    assert torch.equal(out, (8 * taps(8) + 1)[..., None].expand(1, 8, 8, 16)), "the same call with nothing changed runs"


def taps(n):
    """How many of a 3 x 3 p(1,1) kernel's taps lie inside an n x n map, per pixel -> (1, n, n) tensor on the device"""
    side = torch.full((n,), 3.0, device=DEV)
    side[0] = side[-1] = 2.0
    return (side[:, None] * side[None, :])[None]


# ---- pools
def nhwc(y):
    return y.permute(0, 2, 3, 1)


def pool_direct(x, C, mode, out, coff):
    N, H, W, ldx = x.shape
    _lib.call("ps_fid_pool", x, ldx, mode, N, H, W, C, out, out.size(3), coff)


@pytest.mark.parametrize("C", [4, 12, 100])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 2), (3, 3), (4, 4), (5, 4)])
def test_pools_on_small_maps(H, W, C):
    torch.cuda.set_device(DEV)
    N = 3
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(100 * H + 10 * W + C)).to(DEV)
    xc = x.permute(0, 3, 1, 2)
    wide = torch.full((N, H, W, C + 12), float("nan"), device=DEV)       # ldx > C: NaN in the channels the pool does not read
    wide[..., :C] = x
    refs = {fid.MAX_S1: lambda v: F.max_pool2d(v, 3, 1, 1), fid.AVG_S1: lambda v: F.avg_pool2d(v, 3, 1, 1, count_include_pad=False),
            fid.MEAN: lambda v: v.mean((2, 3), keepdim=True)}
    if H >= 3 and W >= 3:
        refs[fid.MAX_S2] = lambda v: F.max_pool2d(v, 3, 2)
    else:
        with pytest.raises(ValueError, match="too small for a 3 x 3 pool"):
            fid.pool(x, fid.MAX_S2)
        out = torch.full((N, 1, 1, C), SENTINEL, device=DEV)
        with pytest.raises(RuntimeError, match="ps_fid_pool failed.*PS_FID_MAX_S2 takes maps of 3 x 3 and more"):
            pool_direct(x, C, fid.MAX_S2, out, 0)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    for mode, fn in refs.items():
        got = fid.pool(x, mode)
        assert tuple(got.shape) == (N,) + fid.pool_shape(mode, H, W) + (C,)
        if mode in (fid.MAX_S1, fid.MAX_S2):
            assert torch.equal(got, nhwc(fn(xc))), mode
        else:
            want = fn(xc.double())
            err, ref = float((nhwc(want) - got.double()).abs().max()), float((want - fn(xc).double()).abs().max())
            print(f"pool mode {mode} {H}x{W}x{C}: kernel {err:.3e}  torch fp32 {ref:.3e}")
            assert err <= 4 * ref, (mode, err, ref)
        # the entry point itself: a wider input map, a channel offset of a wider output map
        out = torch.full(tuple(got.shape[:3]) + (8 + C + 4,), SENTINEL, device=DEV)
        pool_direct(wide, C, mode, out, 8)
        assert same_bits(out[..., 8:8 + C], got), mode
        assert bool((out[..., :8] == SENTINEL).all()) and bool((out[..., 8 + C:] == SENTINEL).all()), mode


# ---- the input pass
def input_mirror(a):
    """k_fid_input restated in float32 numpy, one rounding per operation: a (B, 3, H, W) float32 in [0, 1] -> (B, 3, 299, 299)"""
    f = np.float32
    H, W = a.shape[2:]
    if (H, W) == (299, 299):
        return a * f(2) - f(1)
    o = np.arange(299, dtype=np.float32) + f(0.5)
    fy, fx = np.maximum(f(H) / f(299) * o - f(0.5), f(0)), np.maximum(f(W) / f(299) * o - f(0.5), f(0))
    y0, x0 = np.minimum(fy.astype(np.int32), H - 1), np.minimum(fx.astype(np.int32), W - 1)
    y1, x1 = y0 + (y0 < H - 1), x0 + (x0 < W - 1)
    ly1, lx1 = (fy - y0.astype(np.float32))[:, None], fx - x0.astype(np.float32)
    ly0, lx0 = f(1) - ly1, f(1) - lx1
    top, bot = a[:, :, y0], a[:, :, y1]
    v = ly0 * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1 * (lx0 * bot[..., x0] + lx1 * bot[..., x1])
    assert v.dtype == np.float32
    return v * f(2) - f(1)


INPUT_SIZES = [(1, 1), (2, 3), (598, 598), (300, 298), (1000, 37)]
EXACT_AS_TORCH = {(598, 598)}       # the sizes on which the kernel's bits are those of torch's fp32 CPU resize (MEASURED)


@pytest.mark.parametrize("H,W", INPUT_SIZES)
def test_input_pass_sources(H, W):
    torch.cuda.set_device(DEV)
    a = np.random.RandomState(1000 * H + W).rand(2, 3, H, W).astype(np.float32)
    out = fid.input_pass(t(a))
    assert tuple(out.shape) == (2, 299, 299, 4) and bool((out[..., 3] == 0).all())
    got = out[..., :3].permute(0, 3, 1, 2).cpu()
    assert same_bits(got, torch.from_numpy(input_mirror(a))), "the formula of the kernel's header, rounding for rounding"
    # the corners: along an axis where the source is no larger than the output, the first and last outputs read one source row
    # (column) alone, twice, with weights that sum to 1: a corner output is what the kernel's formula gives on a source whose every
    # row (column) is that one.  Where both axes are so, it is 2 a - 1 of the corner pixel a < 1: bit for bit at the first corner
    # (weights 1 and 0); at the others l0 a + l1 a is within 4 x 2^-25 of a (l0 = 1 - l1, two products and a sum, each rounded by
    # at most 2^-25), the second axis adds as much, doubling doubles it and the subtraction rounds once more: 17 x 2^-25.
    for oy, sy in ((0, 0), (298, H - 1)):
        for ox, sx in ((0, 0), (298, W - 1)):
            ends = a
            if H <= 299:
                ends = np.broadcast_to(ends[:, :, sy:sy + 1], a.shape)
            if W <= 299:
                ends = np.broadcast_to(ends[:, :, :, sx:sx + 1], a.shape)
            assert np.array_equal(got[:, :, oy, ox].numpy(), input_mirror(np.ascontiguousarray(ends))[:, :, oy, ox]), (oy, ox)
            if H <= 299 and W <= 299:
                assert np.abs(got[:, :, oy, ox].numpy() - (2 * a[:, :, sy, sx].astype(np.float64) - 1)).max() <= 17 * 2.0 ** -25, (oy, ox)
    if H <= 299 and W <= 299:
        assert np.array_equal(got[:, :, 0, 0].numpy(), a[:, :, 0, 0] * np.float32(2) - np.float32(1)), "weights 1 and 0 at the first corner"
    if (H, W) == (598, 598):       # an exact 2 x downsample: every output is the mean of its 2 x 2 block
        blocks = a.astype(np.float64).reshape(2, 3, 299, 2, 299, 2).mean((3, 5))
        # the weights are 0.5 (exact products): two inner sums rounded by 2^-25 and halved, the outer sum, doubled, the subtraction
        assert np.abs(got.double().numpy() - (2 * blocks - 1)).max() <= 5 * 2.0 ** -25
    src = torch.from_numpy(a)
    lib = 2 * F.interpolate(src, size=(299, 299), mode="bilinear", align_corners=False) - 1
    want = 2 * F.interpolate(src.double(), size=(299, 299), mode="bilinear", align_corners=False) - 1
    exact = torch.equal(got, lib)
    ulps = float((got - lib).abs().max()) * 2.0 ** 24          # in ulps of a value in [0.5, 1)
    err, ref = float((got.double() - want).abs().max()), float((lib.double() - want).abs().max())
    print(f"input {H}x{W}: equal to torch's fp32 on the CPU {exact}, largest difference {float((got - lib).abs().max()):.3e} "
          f"({ulps:.0f} ulp of [0.5, 1)); against fp64 kernel {err:.3e}  torch fp32 {ref:.3e}")
    if (H, W) in EXACT_AS_TORCH:
        assert exact
    else:
        assert err <= 4 * ref, (err, ref)


def test_input_pass_reads_views_in_place():
    torch.cuda.set_device(DEV)
    rs = np.random.RandomState(41)
    big = t(rs.rand(2, 3, 80, 60).astype(np.float32))
    crop = big[:, :, 3:67, 5:45]
    assert not crop.is_contiguous() and same_bits(fid.input_pass(crop), fid.input_pass(crop.contiguous())), "a crop view"
    last = big.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not last.is_contiguous() and same_bits(fid.input_pass(last), fid.input_pass(big)), "channels-last storage"
    big8 = t(rs.randint(0, 256, size=(2, 3, 80, 60)).astype(np.uint8))
    crop8 = big8[:, :, 3:67, 5:45]
    assert not crop8.is_contiguous() and same_bits(fid.input_pass(crop8), fid.input_pass(crop8.contiguous())), "a uint8 crop"
    host = crop8.cpu().float().div(255)             # TF.to_tensor's true division, on the host
    assert same_bits(fid.input_pass(crop8), fid.input_pass(host.to(DEV))), "uint8 is x / 255"
