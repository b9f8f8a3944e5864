"""GPU: the glue between the refinement decoder's convolution kernels -- the elementwise passes of csrc/nets.hip at their edges and
every route of networks/architectures.py:ResNet_Block.forward -- against fp64 on the host.

A convolution bias reaches a block's output by five routes (folded into the next norm's shift, added by the split-fp16 kernel, carried
through the pooling with the share inside / 9 of its window, added by the up-sampling pass, added by ps_add_bias_nhwc_f32).  The block
tests multiply every bias by ten, so that one added twice, dropped, or carried without its share is an error of the output's own order;
the reference is the block itself, deep-copied to fp64 on the host, with the same noise draws.  The yardstick is err32, the error of the
block's own fp32 forward on the host against that fp64 output (both as max |y - ref| / max |ref|): a GPU result passes within K * err32.
K = 10 is what test_conv3x3_on_the_fp16_pipe_against_an_fp64_convolution sets on the loosest kernel a block runs.

Measured on the MI355X (printed by the tests): MEASURED_MAXIMA below."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.networks import architectures as A, get_decoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED_MAXIMA = """
err / err32 per block 0..7 (err32 between 1.2e-7 and 4.2e-7; the largest err 7.0e-7 of the output's largest magnitude)
  f16x3, (2, C, 16, 32), channels_last   2.10 2.31 3.30 4.67 2.17 1.92 4.09 1.24
  fp32,  (2, C, 16, 32), channels_last   0.88 0.68 0.58 0.79 0.65 0.53 1.08 0.92    (MIOpen picks its algorithm per run: +- 0.3)
  f16x3, (2, C, 18, 34), channels_last   1.13 0.96 1.05 2.75 1.45 1.01 1.22 1.37
  f16x3, (1, C, 15, 17), channels_last   0.82 1.19 1.09 1.23 0.77 0.70 1.10 1.17
  f16x3, (2, C, 16, 32), NCHW            1.08 1.05 0.71 0.86 1.23 0.91 1.55 0.96
whole decoder at 64 x 64: f16x3 err 1.17e-6, err32 6.6e-7, ratio 1.78; fp32 err 4.8e-7, ratio 0.73
Two split-fp16 convolutions in series stay below 5: K = 10 holds for both modes.
"""

K = 10.0
CL = torch.channels_last


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _nhwc(t):
    """A host NCHW tensor on the device in channels_last storage."""
    return t.to(DEV).contiguous(memory_format=CL)


def _close(got, want64, atol, msg):
    np.testing.assert_allclose(got.double().cpu().numpy(), want64.numpy(), rtol=1e-6, atol=atol, err_msg=msg)


# ---- 2. the elementwise passes of csrc/nets.hip ----------------------------------------------------------------------------------------
def _pool(a, b, bias, post):
    """ps_pool_add_post_nhwc_f32 through the C ABI on channels_last device tensors (b, bias, post may be None)."""
    B, C, H, W = a.shape
    out = torch.full((B, C, H // 2, W // 2), float("nan"), device=DEV).contiguous(memory_format=CL)
    _lib.check(_lib.lib().ps_pool_add_post_nhwc_f32(_p(a), _p(b), _p(bias), _p(post), B, H, W, C, out.data_ptr(), _st()), "ps_pool_add_post_nhwc_f32")
    return out


def _pool64(a, b, bias, post):
    """avg_pool2d(a + bias, 3, 2, 1) + avg_pool2d(b, 3, 2, 1) + post in fp64 (count_include_pad, torch's default: the padding stays zero,
    so a bias reaches a border pixel with the share of its window that lies inside the image)."""
    a = a.double()
    if bias is not None:
        a = a + bias.double().view(1, -1, 1, 1)
    want = F.avg_pool2d(a, 3, 2, 1)
    if b is not None:
        want = want + F.avg_pool2d(b.double(), 3, 2, 1)
    return want if post is None else want + post.double()


@pytest.mark.parametrize("shape", [(2, 8, 2, 2), (1, 4, 2, 6), (3, 64, 16, 24)])
def test_pooling_with_a_post_term_against_fp64(shape):
    """ps_pool_add_post_nhwc_f32 with every combination of b, bias and post given or NULL -- post is the pool-first, convolve-a-quarter
    route of the Down blocks, which no test called outside a decoder pass.  The bias is of order 1 and constant in sign per channel, so
    the top row and left column, where it arrives as 6/9 (4/9 in the corner) of itself, are 0.3-0.6 off if it arrives whole.  Tolerances
    of test_block_elementwise_kernels_against_torch; the last add is a plain fp32 add, so out(post) == out(no post) + post bit for bit."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(H * W + C)
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    bias = torch.randn(C, generator=g) + torch.where(torch.arange(C) % 2 == 0, 2.0, -2.0)
    post = torch.randn(B, C, H // 2, W // 2, generator=g)
    ad, bd, pd, biasd = _nhwc(a), _nhwc(b), _nhwc(post), bias.to(DEV)
    for use_b in (False, True):
        for use_bias in (False, True):
            plain = _pool(ad, bd if use_b else None, biasd if use_bias else None, None)
            with_post = _pool(ad, bd if use_b else None, biasd if use_bias else None, pd)
            for got, use_post in ((plain, False), (with_post, True)):
                tag = f"{shape} b={use_b} bias={use_bias} post={use_post}"
                want = _pool64(a, b if use_b else None, bias if use_bias else None, post if use_post else None)
                assert got.shape == want.shape and not torch.isnan(got).any(), tag
                _close(got[:, :, 0, :], want[:, :, 0, :], 2e-6, "top row (window share 6/9, 4/9 in the corner) " + tag)
                _close(got[:, :, :, 0], want[:, :, :, 0], 2e-6, "left column (window share 6/9, 4/9 in the corner) " + tag)
                _close(got, want, 2e-6, tag)
            assert torch.equal(with_post, plain + pd), f"{shape} b={use_b} bias={use_bias}: post is not a plain add"


def test_resample_sum_hands_post_to_the_pooling_and_refuses_what_it_cannot():
    """_resample_sum("Down", a, None, bias, post=p): what ResNet_Block.forward calls on its pool-first route."""
    g = torch.Generator().manual_seed(4)
    a, bias, post = torch.randn(3, 64, 16, 24, generator=g), torch.randn(64, generator=g) + 2.0, torch.randn(3, 64, 8, 12, generator=g)
    ad, pd = _nhwc(a), _nhwc(post)
    got = A._resample_sum("Down", ad, None, bias.to(DEV), post=pd)
    assert got.is_contiguous(memory_format=CL)
    _close(got, _pool64(a, None, bias, post), 2e-6, "_resample_sum Down + bias + post")
    with pytest.raises(ValueError, match="pooled shape"):
        A._resample_sum("Down", ad, None, bias.to(DEV), post=pd[:, :, :, :6].contiguous(memory_format=CL))      # wrong shape
    with pytest.raises(ValueError, match="channels_last"):
        A._resample_sum("Down", ad, None, bias.to(DEV), post=post.to(DEV))                                       # NCHW storage
    with pytest.raises(ValueError, match="'Down' only"):
        A._resample_sum("Up", ad, None, bias.to(DEV), post=_nhwc(torch.zeros(3, 64, 32, 48)))


def _up(a, b, bias):
    B, C, H, W = a.shape
    out = torch.full((B, C, 2 * H, 2 * W), float("nan"), device=DEV).contiguous(memory_format=CL)
    _lib.check(_lib.lib().ps_upsample_add_nhwc_f32(_p(a), _p(b), _p(bias), B, H, W, C, out.data_ptr(), _st()), "ps_upsample_add_nhwc_f32")
    return out


@pytest.mark.parametrize("shape", [(1, 8, 1, 5), (2, 4, 7, 1), (65, 4, 256, 2)])
def test_upsampling_of_one_row_one_column_and_more_rows_than_workgroups(shape):
    """ps_upsample_add_nhwc_f32 where both neighbour rows (H = 1) or columns (W = 1) are the clamped pixel itself, and with B * H = 16 640
    rows for 16 384 workgroups (the row loop's second trip), against F.interpolate in fp64."""
    g = torch.Generator().manual_seed(sum(shape))
    a, b, bias = torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape[1], generator=g) + 2.0
    up = lambda t: F.interpolate(t.double(), scale_factor=2, mode="bilinear", align_corners=False)
    ad, bd = _nhwc(a), _nhwc(b)
    for use_b, use_bias in ((False, False), (True, False), (False, True), (True, True)):
        got = _up(ad, bd if use_b else None, bias.to(DEV) if use_bias else None)
        want = up(a) + (up(b) if use_b else 0) + (bias.double().view(1, -1, 1, 1) if use_bias else 0)
        assert not torch.isnan(got).any()
        _close(got, want, 2e-6 if use_bias else 1e-6, f"{shape} b={use_b} bias={use_bias}")


def test_grid_stride_loops_take_their_second_trip():
    """k_affine_relu, k_add_bias and k_pool_add launch at most 8192 workgroups of 256 lanes, one channel quad per lane and trip, and
    k_cat_mask_nhwc as many with one pixel per lane: beyond 2^21 quads (pixels) the loops go round again, which no unit test's shape made
    them do (the largest had 12 288 quads).  Same references and tolerances as the small shapes; cat_mask stays bit for bit."""
    g = torch.Generator(device=DEV).manual_seed(8)
    L = _lib.lib()
    B, C, H, W = 1, 64, 384, 384
    assert B * H * W * C // 4 > 2 ** 21
    x = torch.randn(B, H, W, C, device=DEV, generator=g)                  # (NHWC memory, used as such)
    b = torch.randn(B, H, W, C, device=DEV, generator=g)
    # scale in [0.5, 1.5): |x * scale| stays below 8, so the product is rounded by at most 2^-22 = 2.4e-7 and the difference, below 16, by
    # 4.8e-7: inside the small shapes' atol of 1e-6
    scale, shift = torch.rand(B, C, device=DEV, generator=g) + 0.5, torch.randn(B, C, device=DEV, generator=g)
    bias = torch.randn(C, device=DEV, generator=g) + 2.0
    y = torch.full_like(x, float("nan"))
    _lib.check(L.ps_affine_relu_nhwc_f32(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), B, H * W, C, y.data_ptr(), _st()), "ps_affine_relu_nhwc_f32")
    want = torch.clamp_min(x.cpu().double() * scale.cpu().double().view(B, 1, 1, C) - shift.cpu().double().view(B, 1, 1, C), 0)
    _close(y, want, 1e-6, "affine_relu, second trip")
    y.fill_(float("nan"))
    _lib.check(L.ps_add_bias_nhwc_f32(x.data_ptr(), b.data_ptr(), bias.data_ptr(), B, H * W, C, y.data_ptr(), _st()), "ps_add_bias_nhwc_f32")
    _close(y, x.cpu().double() + b.cpu().double() + bias.cpu().double(), 2e-6, "add_bias, second trip")
    del y, b
    # the pooling's loop runs over OUTPUT quads: 364 x 364 x 16 of them
    H = W = 728
    assert B * (H // 2) * (W // 2) * C // 4 > 2 ** 21
    a = torch.randn(B, C, H, W, device=DEV, generator=g).contiguous(memory_format=CL)
    post = torch.randn(B, C, H // 2, W // 2, device=DEV, generator=g).contiguous(memory_format=CL)
    got = _pool(a, None, bias, post)
    _close(got, _pool64(a.cpu(), None, bias.cpu(), post.cpu()), 2e-6, "pool_add_post, second trip")
    del a, post, got
    B, H, W = 9, 512, 512
    assert B * H * W > 2 ** 21
    img = torch.randn(B, 3, H, W, device=DEV, generator=g)
    bg = torch.rand(B, H, W, device=DEV, generator=g) > 0.4
    out = torch.full((B, H, W, 4), float("nan"), device=DEV)
    _lib.check(L.ps_cat_mask_nhwc_f32(img.data_ptr(), bg.data_ptr(), B, H, W, out.data_ptr(), _st()), "ps_cat_mask_nhwc_f32")
    assert torch.equal(out.permute(0, 3, 1, 2), torch.cat((img, (~bg).unsqueeze(1).float()), 1))


def test_affine_relu_of_single_pixel_frames_takes_each_samples_own_row():
    """ps_affine_relu_nhwc_f32 with HW = 1 and B = 5: the frame index i / per_frame4 changes every C / 4 lanes; every sample has its own
    scale and shift row (a kernel that read row 0 for all of them, or indexed frames by pixels, is off by order 1)."""
    g = torch.Generator().manual_seed(6)
    B, C = 5, 8
    x, scale, shift = torch.randn(B, 1, C, generator=g), torch.rand(B, C, generator=g) + 0.5, torch.randn(B, C, generator=g)
    y = torch.full((B, 1, C), float("nan"), device=DEV)
    xd, sc, sh = x.to(DEV), scale.to(DEV), shift.to(DEV)
    _lib.check(_lib.lib().ps_affine_relu_nhwc_f32(xd.data_ptr(), sc.data_ptr(), sh.data_ptr(), B, 1, C, y.data_ptr(), _st()), "ps_affine_relu_nhwc_f32")
    want = torch.clamp_min(x.double() * scale.double().view(B, 1, C) - shift.double().view(B, 1, C), 0)
    assert (want > 0).sum() > B and (want == 0).sum() > B       # (both sides of the ReLU)
    _close(y, want, 1e-6, "affine_relu HW = 1")


# ---- 3. every route of ResNet_Block.forward ---------------------------------------------------------------------------------------------
def _decoder(seed):
    """get_decoder(syn.network_opts()) on the host, filled by syn.fill_state_dict, every convolution bias times ten."""
    dec = get_decoder(syn.network_opts())
    shapes = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, seed).items()}
    scaled = [k for k in sd if k.endswith(".bias")]
    assert len(scaled) == 8 * 2 + 6          # two 3 x 3 layers per block, six projections
    for k in scaled:
        sd[k] = sd[k] * 10
    dec.load_state_dict(sd, strict=True)
    return dec.eval()


def _rel(y, ref64):
    return (y.double().cpu() - ref64).abs().max().item() / ref64.abs().max().item()


class _Blocks:
    """The eight blocks three times -- fp32 on the host, fp64 on the host (the reference), fp32 on the device -- and, per (block, shape), the
    input, the noise draws, the fp64 output and err32, computed once and shared."""

    def __init__(self):
        dec = _decoder(3)
        self.cpu = list(dec.eblocks)
        self.ref = [copy.deepcopy(b).double() for b in self.cpu]
        self.gpu = [copy.deepcopy(b).to(DEV) for b in self.cpu]
        self.cases = {}

    def case(self, i, shape):
        if (i, shape) not in self.cases:
            B, H, W = shape
            C = self.cpu[i].ch_a[2].in_channels
            g = torch.Generator().manual_seed(100 * i + H)
            x = torch.randn(B, C, H, W, generator=g)
            noise = [torch.randn(B, A.NOISE_SZ, generator=g) for _ in range(2)]          # (different rows per sample)
            with torch.no_grad():
                ref = self.ref[i](x.double(), [n.double() for n in noise])
                err32 = _rel(self.cpu[i](x, noise), ref)
            assert ref.dtype == torch.float64 and 2e-8 < err32 < 1e-6, err32
            self.cases[(i, shape)] = (x, noise, ref, err32)
        return self.cases[(i, shape)]


@pytest.fixture(scope="module")
def blocks():
    return _Blocks()


_IGNORED = ("ps_conv3x3_f16x3_packed_bytes", "ps_conv3x3_f16x3_pack")    # (a weight is packed at its first use only)


def _spy(monkeypatch):
    """Record every entry point the package calls through _lib.call as (name, indices of the arguments that are None, arguments)."""
    calls, real = [], _lib.call

    def call(name, *args, **kw):
        if name not in _IGNORED:
            calls.append((name, tuple(j for j, a in enumerate(args) if a is None), args))
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, "call", call)
    return calls


def _forward(blocks, i, mode, shape, layout):
    x, noise, ref, err32 = blocks.case(i, shape)
    xd = x.to(DEV)
    if layout == "nhwc":
        xd = xd.contiguous(memory_format=CL)
    else:
        assert xd.is_contiguous() and not xd.is_contiguous(memory_format=CL)
    with torch.no_grad(), A.decoder_conv(mode):
        y = blocks.gpu[i](xd, [n.to(DEV) for n in noise])
        A.check_f16x3_overflow(xd.device)
    assert y.shape == ref.shape
    return _rel(y, ref), err32


# (mode, (B, H, W), storage of the input): 16 x 32 is the smallest size the split-fp16 kernel takes (the Down blocks pool it to 8 x 16);
# 18 x 34 is even, but that kernel refuses it -- the convolutions go through torch while the pool-first route and its post term stay;
# 15 x 17 is odd: _resample_sum goes through torch and the pool-first route is not taken; NCHW storage: nothing of csrc/nets.hip applies
CASES = [("f16x3", (2, 16, 32), "nhwc"), ("fp32", (2, 16, 32), "nhwc"), ("f16x3", (2, 18, 34), "nhwc"), ("f16x3", (1, 15, 17), "nhwc"),
         ("f16x3", (2, 16, 32), "nchw")]
_ID = lambda c: "%s-%dx%dx%d-%s" % (c[0], *c[1], c[2])


@pytest.mark.parametrize("case", CASES, ids=_ID)
@pytest.mark.parametrize("i", range(8))
def test_block_on_the_gpu_against_the_block_in_fp64(blocks, i, case):
    """Each of the decoder's eight blocks (4 -> 64, 64 -> 128 and 128 -> 256 Down, 256 -> 256, 256 -> 128 and 128 -> 128 Up, 128 -> 128,
    128 -> 3), biases times ten, per-sample noise: error against the fp64 block within K * err32 (module docstring)."""
    mode, shape, layout = case
    err, err32 = _forward(blocks, i, mode, shape, layout)
    print(f"block {i} {_ID(case)}: err {err:.3e} err32 {err32:.3e} ratio {err / err32:.2f}")
    assert err <= K * err32, (err, err32, err / err32)


NA, AR, ADD = "ps_noise_affine_f32", "ps_affine_relu_nhwc_f32", "ps_add_bias_nhwc_f32"
F16, TIN, TOUT = "ps_conv3x3_f16x3_ex_nhwc", "ps_conv3x3_thin_in_f16x3_nhwc", "ps_conv3x3_thin_out_nhwc_f32"
TAKES, C1, POOL, UP = "ps_conv1x1_takes", "ps_conv1x1_nhwc_f32", "ps_pool_add_post_nhwc_f32", "ps_upsample_add_nhwc_f32"
# Arguments that may be NULL, by position: NA (noise, wg, wb, mean, var, PEND, ...); F16 (x, scale, shift, packed, BIAS, RES, ...);
# POOL (a, B, BIAS, POST, ...); UP (a, B, BIAS, ...); ADD (a, b, BIAS, ...)
_NORM1, _NORM2 = (NA, (5,)), (NA, ())            # the first norm has no pending bias; the second folds the first convolution's into shift
_PROJ = [(TAKES, ()), (C1, ())]                  # the 1 x 1 projection of the other branch (its bias comes back separate)
_KIND = ["first", "down", "down", "same", "up", "up", "same", "last"]
ROUTES = {
    # split-fp16 convolutions, norm + ReLU applied as they stage their input
    ("f16x3", (2, 16, 32)): {
        "first": [_NORM1, (TIN, ())] + _PROJ + [_NORM2, (F16, ())],               # res and the summed bias go out with the convolution
        # pool x, convolve a quarter of the pixels, pool the main branch with both biases riding through and the projection as post
        "down": [_NORM1, (F16, (4, 5)), (POOL, (1, 2, 3))] + _PROJ + [_NORM2, (F16, (4, 5)), (POOL, (1,))],
        "same": [_NORM1, (F16, (4, 5)), _NORM2, (F16, ())],                      # res = x, bias = the second convolution's own
        "up": [_NORM1, (F16, (4, 5))] + _PROJ + [_NORM2, (F16, (4,)), (UP, (1,))],  # the sum of the branches up-sampled once, biases there
        # 128 -> 3: the thin kernel, then three channels -- nothing of csrc/nets.hip takes them: norm, 3 -> 3 and the sum through torch
        "last": [_NORM1, (TOUT, ())] + _PROJ + [_NORM2],
    },
    # everything through torch's convolutions, the bias split off where the output has a multiple of 4 channels
    ("fp32", (2, 16, 32)): {
        "first": [_NORM1, (AR, ()), _NORM2, (AR, ()), (ADD, ())],
        "down": [_NORM1, (AR, ()), _NORM2, (AR, ()), (POOL, (3,))],
        "same": [_NORM1, (AR, ()), _NORM2, (AR, ()), (ADD, ())],
        "up": [_NORM1, (AR, ()), _NORM2, (AR, ()), (UP, ())],
        "last": [_NORM1, (AR, ())],
    },
    ("f16x3", (2, 18, 34)): {
        "first": [_NORM1, (AR, ())] + _PROJ + [_NORM2, (AR, ()), (ADD, ())],
        "down": [_NORM1, (AR, ()), (POOL, (1, 2, 3))] + _PROJ + [_NORM2, (AR, ()), (POOL, (1,))],
        "same": [_NORM1, (AR, ()), _NORM2, (AR, ()), (ADD, ())],
        "up": [_NORM1, (AR, ())] + _PROJ + [_NORM2, (AR, ()), (UP, ())],
        "last": [_NORM1, (AR, ())] + _PROJ + [_NORM1],                         # (128 -> 3 through torch keeps its bias: none pending)
    },
    ("f16x3", (1, 15, 17)): {
        "first": [_NORM1, (AR, ())] + _PROJ + [_NORM2, (AR, ()), (ADD, ())],
        "down": [_NORM1, (AR, ())] + _PROJ + [_NORM2, (AR, ())],                # full-size projection; both poolings and their sum: torch
        "same": [_NORM1, (AR, ()), _NORM2, (AR, ()), (ADD, ())],
        "up": [_NORM1, (AR, ())] + _PROJ + [_NORM2, (AR, ()), (UP, ())],
        "last": [_NORM1, (AR, ())] + _PROJ + [_NORM1],
    },
}


@pytest.mark.parametrize("case", CASES[:4], ids=_ID)
@pytest.mark.parametrize("i", range(8))
def test_block_takes_the_route_written_down_for_it(blocks, i, case, monkeypatch):
    """Which entry points a block runs, in order, and which of their optional pointers are NULL: a silent change of route -- a kernel
    no longer taken, a bias handed to another pass -- fails here even where both routes compute the same numbers."""
    mode, shape, _ = case
    B, H, W = shape
    calls = _spy(monkeypatch)
    _forward(blocks, i, mode, shape, "nhwc")
    got = [(name, nulls) for name, nulls, _ in calls]
    print(f"block {i} {_ID(case)}: {got}")
    assert got == ROUTES[(mode, shape)][_KIND[i]]
    pooled = mode == "f16x3" and _KIND[i] == "down" and H % 2 == 0
    for name, _, args in calls:
        if name == C1:      # (x, w, npix, Ci, Co, y): the Down blocks' projection runs on the POOLED pixels
            assert args[2] == (B * (H // 2) * (W // 2) if pooled else B * H * W)
        if name == POOL:    # (a, b, bias, post, B, H, W, C, out): x alone is pooled at its own width, the main branch at the block's
            alone = args[1] is None and args[3] is None
            assert args[4:8] == (B, H, W, blocks.cpu[i].ch_a[2].in_channels if alone else blocks.cpu[i].ch_a[5].out_channels)


def test_block_with_nchw_input_runs_nothing_of_the_channels_last_kernels(blocks, monkeypatch):
    calls = _spy(monkeypatch)
    _forward(blocks, 1, "f16x3", (2, 16, 32), "nchw")
    assert [(name, nulls) for name, nulls, _ in calls] == [_NORM1, _NORM1]      # (torch's convolutions keep their biases)


@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
def test_whole_decoder_at_its_smallest_size_against_fp64(mode):
    """The eight blocks in series at 64 x 64 (16 x 16 at the bottom, the smallest the split-fp16 kernel takes), B = 2, ragged background
    mask, biases times ten, predict_residual as the options set it, and tanh replaced by the identity so that it does not squash the error:
    against the deep copy in fp64 on the host, same yardstick as the blocks."""
    dec = _decoder(5)
    dec.norm = torch.nn.Identity()
    assert dec.opt.predict_residual
    S, B = 64, 2
    x = torch.from_numpy(syn.image(11, B, 3, S))
    bgm = torch.from_numpy(syn.background_masks(S)["ragged"])
    bgm = torch.stack([bgm, ~bgm.flip(1)])
    g = torch.Generator().manual_seed(12)
    noise = [torch.randn(B, A.NOISE_SZ, generator=g) for _ in range(dec.n_noise())]
    with torch.no_grad():
        ref = copy.deepcopy(dec).double()(x.double(), bgm, noise=[n.double() for n in noise])
        err32 = _rel(dec(x, bgm, noise=noise), ref)
        dec = dec.to(DEV)
        with A.decoder_conv(mode):
            y = dec(x.to(DEV), bgm.to(DEV), noise=[n.to(DEV) for n in noise])
            A.check_f16x3_overflow(torch.device(DEV))
    err = _rel(y, ref)
    print(f"decoder {mode}: err {err:.3e} err32 {err32:.3e} ratio {err / err32:.2f}")
    assert ref.shape == (B, 3, S, S) and 2e-8 < err32 < 1e-6
    assert err <= K * err32, (err, err32, err / err32)
