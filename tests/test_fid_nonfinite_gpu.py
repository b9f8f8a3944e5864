"""GPU: non-finite values through the FID passes (csrc/fid.hip).  The contract is torch's, as FIDInception.torch_forward has it:
relu and the max pools hand a NaN on.  A NaN in x reaches exactly the outputs of ps_fid_conv whose receptive field holds it, in
every output channel, and no other output moves a bit; +inf under positive weights gives +inf, -inf gives 0; the max pools equal
F.max_pool2d on a map with NaN and -inf; the averaging pools hand NaN on; a NaN pixel in one image of a batch gives that image a
feature row with NaN, as net.torch_forward does, and leaves the other rows' bits alone."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fid_edge_cases as E
import fid_ref64 as R
from pixelsynth_amd import fid, synthetic as syn
from pixelsynth_amd.networks import inception as I
from test_fid_conv_edges_gpu import DEV, conv_fresh, nhwc, pack, same_bits, t

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")

# cases of the table with scalar tails at both tile widths, stride 2 with padding, S = 4 and 5, a map narrower than the kernel
CASES = [8, 9, 10, 13, 17, 24]


def spots(case, N):
    """(image, h, w, channel) of an interior pixel of image 0 and of the last pixel of the last image"""
    Ci, H, W = case[5], case[9], case[10]
    return [(0, H // 2, W // 2, 1), (N - 1, H - 1, W - 1, Ci - 1)]


def field(case, N, where):
    """-> (N, Ho, Wo, 1) bool on the CPU: the outputs whose receptive field holds a pixel of `where`"""
    KH, KW, s, ph, pw = case[:5]
    ind = torch.zeros(N, 1, case[9], case[10], dtype=torch.float64)
    for n, h, w, _ in where:
        ind[n, 0, h, w] = 1
    return nhwc(F.conv2d(ind, torch.ones(1, 1, KH, KW, dtype=torch.float64), None, s, (ph, pw)) > 0)


@pytest.mark.parametrize("k", CASES, ids=[E.name(E.CASES[k]) for k in CASES])
def test_conv_hands_nan_to_its_receptive_field_alone(k):
    case = E.CASES[k]
    Co, N = case[7], case[8]
    x, w, b = E.randn_operands(case, 900 + k)
    layer = pack(w, b, case)
    clean = conv_fresh(t(x), layer).cpu()
    where = spots(case, N)
    for n, h, c_w, c in where:
        x[n, h, c_w, c] = np.nan
    hit = field(case, N, where).expand(-1, -1, -1, Co)
    assert hit.any() and not hit.all() or E.pixels(case) == 1
    got = conv_fresh(t(x), layer).cpu()
    assert torch.equal(got.isnan(), hit), f"NaN in {int(got.isnan().sum())} outputs, {int(hit.sum())} hold it in their field"
    assert same_bits(torch.where(hit, clean, got), clean), "the other outputs keep the clean run's bits"
    want = E.reference(x, w, b, case)
    assert torch.equal(want.isnan(), hit), "relu(conv2d) in fp64"


@pytest.mark.parametrize("k", CASES, ids=[E.name(E.CASES[k]) for k in CASES])
def test_conv_on_infinities(k):
    case = E.CASES[k]
    Co, N = case[7], case[8]
    x, w, b = E.randn_operands(case, 950 + k)
    w = np.abs(w) + np.float32(0.01)
    layer = pack(w, b, case)
    clean = conv_fresh(t(x), layer).cpu()
    where = spots(case, N)
    hit = field(case, N, where).expand(-1, -1, -1, Co)
    for value, want in ((INF, INF), (-INF, 0.0)):
        for n, h, c_w, c in where:
            x[n, h, c_w, c] = value
        got = conv_fresh(t(x), layer).cpu()
        assert bool((got[hit] == want).all()), (value, got[hit].unique()[:8])
        assert same_bits(torch.where(hit, clean, got), clean), value


def equal_or_both_nan(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize("H,W,C", [(7, 6, 8), (3, 3, 4), (9, 5, 100)])
def test_pools_on_nan_and_minus_infinity(H, W, C):
    torch.cuda.set_device(DEV)
    x = torch.randn(2, H, W, C, generator=torch.Generator().manual_seed(H))
    x[0, :2, :2, :] = -INF                   # the 3 x 3 p(1,1) window of pixel (0, 0) holds nothing else
    x[1, 1, 0, 0] = -INF
    x[0, H - 1, W - 1, 1] = NAN              # the last pixel of a map
    x[1, H // 2, W // 2, C - 1] = NAN        # an interior one
    x[1, 0, 1, 2] = NAN
    x[1, 0, 2, 2] = 50.0                     # a larger value after a NaN in the same window
    xc = x.permute(0, 3, 1, 2)
    for mode, fn in ((fid.MAX_S2, lambda v: F.max_pool2d(v, 3, 2)), (fid.MAX_S1, lambda v: F.max_pool2d(v, 3, 1, 1))):
        want, got = nhwc(fn(xc)), fid.pool(x.to(DEV), mode).cpu()
        assert want.isnan().any() and bool((want == -INF).any() or mode == fid.MAX_S2)
        assert torch.equal(got.isnan(), want.isnan()), (mode, int(got.isnan().sum()), int(want.isnan().sum()))
        assert equal_or_both_nan(got, want), mode
    # the averages: NaN wherever the window (the map) holds one, the other outputs as without it
    nan = x.isnan()
    finite = torch.where(nan | x.isinf(), torch.zeros(()), x)
    dirty = torch.where(nan, x, finite)
    hit = nhwc(F.max_pool2d(nan.permute(0, 3, 1, 2).float(), 3, 1, 1)) > 0
    got, clean = fid.pool(dirty.to(DEV), fid.AVG_S1).cpu(), fid.pool(finite.to(DEV), fid.AVG_S1).cpu()
    assert torch.equal(got.isnan(), hit) and same_bits(torch.where(hit, clean, got), clean)
    hit = nan.any(1, keepdim=True).any(2, keepdim=True)
    got, clean = fid.pool(dirty.to(DEV), fid.MEAN).cpu(), fid.pool(finite.to(DEV), fid.MEAN).cpu()
    assert hit.any() and not hit.all()
    assert torch.equal(got.isnan(), hit) and same_bits(torch.where(hit, clean, got), clean)


def test_a_nan_pixel_reaches_its_own_feature_row_alone():
    torch.cuda.set_device(DEV)
    net = I.FIDInception(weights={k: torch.from_numpy(v) for k, v in R.weights().items()}, use_gpu=True)
    a = syn.metric_pair(98, 3, 3, 64, 64)[1].copy()
    clean = fid.inception_features(net, t(a))
    assert bool(clean.isfinite().all())
    a[1, 2, 30, 17] = np.nan
    got = fid.inception_features(net, t(a))
    with torch.no_grad():
        lib = net.torch_forward(t(a))
    print(f"one NaN pixel in image 1: NaN in {int(got[1].isnan().sum())} of 2048 features on the HIP path, "
          f"{int(lib[1].isnan().sum())} through torch")
    assert bool(lib[1].isnan().any()) and bool(lib[[0, 2]].isfinite().all()), "the torch formula"
    assert bool(got[1].isnan().any()), "a row with a NaN pixel must not come out finite"
    assert same_bits(got[[0, 2]], clean[[0, 2]]), "the other images' rows keep their bits"
