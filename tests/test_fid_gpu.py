"""GPU: the FID passes (csrc/fid.hip) and inception_features on the HIP path: ps_fid_conv on every distinct convolution of the network
against an fp64 convolution of the same operands, the pools and the input pass against torch, the features against the fp64
restatement's record (tests/golden/fid.npz), bit-level properties (run to run, batch split, uint8 = fp32 of x / 255, channels-last =
contiguous), FID of two image sets against the fp64 record, and the CLI with --inception on one rank and two.

Bounds: a kernel's largest error against fp64 is at most 4 x the error of torch's own fp32 operator (library code) on the same
operands, measured in the same test; the features' at most 4 x err32, the restatement's fp32 error recorded in fid.npz.
Measured maxima on the MI355X (printed by the tests): MEASURED_MAXIMA below."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_ref64 as R
from pixelsynth_amd import fid, synthetic as syn
from pixelsynth_amd.networks import inception as I
from test_metrics_gpu import _cli, _png_dirs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEASURED_MAXIMA = """one run on the MI355X (torch's own figures move a little from run to run, the kernels' do not):
fid conv: 43 shapes, largest kernel / torch error ratio 1.19 at (1, 1, 1, 0, 0, 256, 48, 35, 35)
pool AVG_S1, kernel = torch fp32: 2.732e-07 (147x147x64), 2.550e-07 (35x35x288), 2.119e-07 (17x17x768), 2.293e-07 (8x8x2048), 1.391e-07 (9x5x8)
pool MEAN, kernel / torch fp32: 8.746e-10 / 3.600e-09, 2.926e-09 / 1.716e-08, 7.447e-09 / 3.241e-08, 1.473e-08 / 4.628e-08, 1.100e-08 / 3.161e-08
input, kernel / torch fp32: 6.240e-06 / 6.141e-06 (256x256), 1.572e-05 / 1.572e-05 (180x320), 1.644e-05 / 1.644e-05 (512x300), 2.181e-06 / 2.181e-06 (64x40)
features against fp64, hip / torch / bound: noise299 2.43e-05 / 4.84e-05 / 9.7e-05, blur299 7.12e-06 / 1.21e-05 / 4.94e-05, blur256 1.25e-05 / 1.74e-05 / 5.1e-05
FID of two 64-image sets: HIP features 35.595966735, fp64 35.595908725, relative 1.630e-06 (the restatement's fp32: 1.173e-06)"""


@pytest.fixture(scope="module")
def net():
    torch.cuda.set_device(DEV)
    return I.FIDInception(weights={k: torch.from_numpy(v) for k, v in R.weights().items()}, use_gpu=True)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fid.npz"))


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def conv_shapes():
    """Every distinct (KH, KW, stride, ph, pw, Ci, Co, H, W) of the network, walked from inception.NETWORK at 299 x 299 (the stem's
    Ci is the padded 4)."""
    specs, seen = I.conv_specs(), []
    shape = (299, 299, 4)

    def step_shape(step, H, W, C):
        if isinstance(step, tuple):
            outs = [step_shape(s, H, W, C) for s in step]
            return outs[0][:2] + (sum(o[2] for o in outs),)
        if step in I.POOLS:
            return ((H - 3) // 2 + 1, (W - 3) // 2 + 1, C) if step == "max2" else (H, W, C)
        ci, co, (kh, kw), s, (ph, pw) = specs[step]
        assert (ci + 3) // 4 * 4 == C, (step, ci, C)
        seen.append((kh, kw, s, ph, pw, C, co, H, W))
        return ((H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1, co)

    for _, branches in I.NETWORK:
        outs = []
        for steps in branches:
            s = shape
            for step in steps:
                s = step_shape(step, *s)
            outs.append(s)
        shape = outs[0][:2] + (sum(o[2] for o in outs),)
    assert shape == (8, 8, 2048) and len(seen) == 94
    return sorted(set(seen))


def test_conv_on_every_shape_of_the_network():
    torch.cuda.set_device(DEV)
    shapes = conv_shapes()
    g = torch.Generator(device="cpu").manual_seed(5)
    worst, failed = (0.0, None), []
    for kh, kw, s, ph, pw, ci, co, H, W in shapes:
        N = 2
        x = torch.randn(N, H, W, ci, generator=g).to(DEV)
        w = (torch.randn(co, ci, kh, kw, generator=g) * (2.0 / (kh * kw * ci)) ** 0.5).to(DEV)
        b = (torch.randn(co, generator=g) * 0.1).to(DEV)
        layer = fid.pack_conv(w, b, s, (ph, pw))
        xc = x.permute(0, 3, 1, 2)
        want = torch.relu(F.conv2d(xc.double(), w.double(), b.double(), s, (ph, pw)))
        lib = torch.relu(F.conv2d(xc, w, b, s, (ph, pw)))
        # into a wider map at a channel offset: the neighbours stay as they were, bit for bit
        Ho, Wo = want.shape[2:]
        out = torch.randn(N, Ho, Wo, co + 12, generator=g).to(DEV)
        before = out.clone()
        fid.conv(x, layer, out, 8)
        got = out[..., 8:8 + co].permute(0, 3, 1, 2)
        assert torch.equal(out[..., :8], before[..., :8]) and torch.equal(out[..., 8 + co:], before[..., 8 + co:])
        assert torch.equal(fid.conv(x, layer), out[..., 8:8 + co]), "the same values without an offset"
        err, ref = float((got.double() - want).abs().max()), float((lib.double() - want).abs().max())
        print(f"conv {kh}x{kw} s{s} p({ph},{pw}) {ci:4d}->{co:3d} {H:3d}x{W:3d}: kernel {err:.3e}  torch fp32 {ref:.3e}  ratio {err / ref:.2f}")
        if err / ref > worst[0]:
            worst = (err / ref, (kh, kw, s, ph, pw, ci, co, H, W))
        if not err <= 4 * ref:
            failed.append((kh, kw, s, ph, pw, ci, co, H, W, err, ref))
    print(f"fid conv: {len(shapes)} shapes, largest kernel / torch error ratio {worst[0]:.2f} at {worst[1]}")
    assert not failed, failed


def test_conv_rejects_what_it_does_not_take():
    torch.cuda.set_device(DEV)
    x = torch.zeros(1, 8, 8, 8, device=DEV)
    layer = fid.pack_conv(torch.zeros(16, 8, 3, 3, device=DEV), torch.zeros(16, device=DEV), 1, (1, 1))
    with pytest.raises(ValueError, match="does not hold channels"):
        fid.conv(x, layer, torch.zeros(1, 8, 8, 20, device=DEV), 8)
    with pytest.raises(RuntimeError, match="ps_fid_conv failed.*multiples of 4"):
        fid.conv(x, layer, torch.zeros(1, 8, 8, 20, device=DEV), 2)
    with pytest.raises(RuntimeError, match="ps_fid_conv failed.*packed weights"):
        fid.conv(x, dict(layer, wp=layer["wp"][:-64]))
    with pytest.raises(RuntimeError, match="ps_fid_conv failed.*stride"):
        fid.conv(x, dict(layer, stride=3))


@pytest.mark.parametrize("H,W,C", [(147, 147, 64), (35, 35, 288), (17, 17, 768), (8, 8, 2048), (9, 5, 8)])
def test_pools(H, W, C):
    torch.cuda.set_device(DEV)
    x = torch.randn(3, H, W, C, generator=torch.Generator().manual_seed(H)).to(DEV)
    xc = x.permute(0, 3, 1, 2)
    nhwc = lambda y: y.permute(0, 2, 3, 1)
    assert torch.equal(fid.pool(x, fid.MAX_S2), nhwc(F.max_pool2d(xc, 3, 2)))
    assert torch.equal(fid.pool(x, fid.MAX_S1), nhwc(F.max_pool2d(xc, 3, 1, 1)))
    out = torch.full((3, H, W, C + 8), 7.0, device=DEV)
    fid.pool(x, fid.MAX_S1, out, 4)
    assert torch.equal(out[..., 4:4 + C], fid.pool(x, fid.MAX_S1)) and bool((out[..., :4] == 7).all()) and bool((out[..., 4 + C:] == 7).all())
    for mode, fn in ((fid.AVG_S1, lambda v: F.avg_pool2d(v, 3, 1, 1, count_include_pad=False)), (fid.MEAN, lambda v: v.mean((2, 3), keepdim=True))):
        want = fn(xc.double())
        err = float((nhwc(want) - fid.pool(x, mode).double()).abs().max())
        ref = float((want - fn(xc).double()).abs().max())
        print(f"pool mode {mode} {H}x{W}x{C}: kernel {err:.3e}  torch fp32 {ref:.3e}")
        assert err <= 4 * ref, (mode, err, ref)


@pytest.mark.parametrize("H,W", [(256, 256), (299, 299), (180, 320), (512, 300), (64, 40)])
def test_input_pass(H, W):
    torch.cuda.set_device(DEV)
    a = t(syn.metric_pair(90 + H, 2, 3, H, W)[1])
    got = fid.input_pass(a)
    assert tuple(got.shape) == (2, 299, 299, 4) and bool((got[..., 3] == 0).all())
    got = got[..., :3].permute(0, 3, 1, 2)
    if (H, W) == (299, 299):
        assert torch.equal(got, a * 2 - 1), "an identity but for 2 x - 1"
        return
    want = 2 * F.interpolate(a.double(), size=(299, 299), mode="bilinear", align_corners=False) - 1
    lib = 2 * F.interpolate(a, size=(299, 299), mode="bilinear", align_corners=False) - 1
    err, ref = float((got.double() - want).abs().max()), float((lib.double() - want).abs().max())
    print(f"input {H}x{W}: kernel {err:.3e}  torch fp32 {ref:.3e}")
    assert err <= 4 * ref, (err, ref)


def test_features_against_the_fp64_record(net, golden):
    worst = {}
    for case in R.CASES:
        x = t(R.case_input(case))
        got = fid.inception_features(net, x)
        assert tuple(got.shape) == (1, 2048) and got.dtype == torch.float32
        f64, bound = golden["f64/" + case[0]], 4 * float(golden["err32/" + case[0]])
        err = float(np.abs(got.cpu().double().numpy() - f64).max())
        with torch.no_grad():
            lib = float(np.abs(net.torch_forward(x).cpu().double().numpy() - f64).max())
        worst[case[0]] = dict(hip=float("%.3g" % err), torch=float("%.3g" % lib), bound=float("%.3g" % bound))
        assert err <= bound, (case[0], err, bound)
        assert torch.equal(net(x), got), "FIDInception.forward on the device is the HIP path"
    print("fid feature error maxima against fp64:", json.dumps(worst))


def test_bit_level_properties(net):
    a = syn.metric_pair(95, 5, 3, 256, 256)[1]
    one = fid.inception_features(net, t(a))
    assert torch.equal(one, fid.inception_features(net, t(a))), "run to run"
    for lo, hi in ((0, 1), (1, 5), (2, 4)):
        assert torch.equal(fid.inception_features(net, t(a[lo:hi])), one[lo:hi]), (lo, hi)
    nhwc = t(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
    assert not nhwc.is_contiguous() and torch.equal(fid.inception_features(net, nhwc), one), "channels-last storage"
    u8 = syn.metric_pair(96, 2, 3, 256, 256, "uint8")[0]
    f32 = torch.from_numpy(u8).float().div(255)                      # TF.to_tensor, on the host
    assert torch.equal(fid.inception_features(net, t(u8)), fid.inception_features(net, f32.to(DEV)))
    assert float(one.std(0).mean()) > 0, "rows differ between images"


def test_passes_are_cut_and_rows_do_not_move(net, monkeypatch):
    a = syn.metric_pair(97, 3, 3, 64, 64)[1]
    one = fid.inception_features(net, t(a))
    monkeypatch.setattr(fid, "_PASS_BYTES", 2 * fid._IMAGE_BYTES)
    assert fid.images_per_pass() == 2
    assert torch.equal(fid.inception_features(net, t(a)), one)


def test_fid_of_two_sets_against_the_fp64_record(net, golden):
    sets = R.fid_sets()
    assert [float(np.asarray(s, np.float64).sum()) for s in sets] == list(golden["fid/sum"])
    rows = [fid.inception_features(net, t(s)) for s in sets]
    got = fid.fid_of_rows(*rows)
    want, rel32 = float(golden["fid/fid64"]), float(golden["fid/rel32"])
    rel = abs(got - want) / want
    print(f"FID of two 64-image sets: HIP features {got:.9f}  fp64 {want:.9f}  relative {rel:.3e}  (restatement's fp32: {rel32:.3e})")
    assert rel <= 4 * rel32


@pytest.fixture(scope="module")
def inception_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("inception") / "pt_inception-2015-12-05-6726825d.pth")
    torch.save({k: torch.from_numpy(v) for k, v in R.weights().items()}, path)
    return path


def _direct_fid(net, a, b):
    rows = [fid.inception_features(net, t(x)).cpu().double().numpy() for x in (a, b)]
    return fid.fid_of_rows(*rows)


def test_cli_fid_line_and_json(tmp_path, inception_file, net):
    dirs, a, b, _ = _png_dirs(tmp_path, n=5, H=96, W=128)
    js = str(tmp_path / "out.json")
    stdout = _cli(["--pred", dirs["pred"], "--gt", dirs["gt"], "--batch", "2", "--json", js, "--inception", inception_file])
    lines = [ln for ln in stdout.splitlines() if " \t " in ln]
    assert [ln.split(" \t ")[0] for ln in lines] == ["PSNR", "SSIM", "FID"]
    want = _direct_fid(net, a, b)
    assert lines[-1] == "FID \t %0.5f" % want, (lines, want)
    doc = json.load(open(js))
    assert doc["fid"] == want and doc["means"]["FID"] == want and list(doc["rows"][0]) == ["index", "psnr", "ssim"]


def test_cli_fid_two_ranks_equal_one(tmp_path, inception_file):
    dirs, _, _, _ = _png_dirs(tmp_path, n=5, H=96, W=128)
    base = ["--pred", dirs["pred"], "--gt", dirs["gt"], "--sampled", dirs["sampled"], "--batch", "2", "--inception", inception_file]
    one, two = str(tmp_path / "one.json"), str(tmp_path / "two.json")
    out1 = _cli(base + ["--json", one])
    out2 = _cli(base + ["--json", two], env={"PS_DRYRUN_ONE_GPU": "1"}, nproc=2)
    d1, d2 = json.load(open(one)), json.load(open(two))
    f1, f2 = (d.pop("fid") for d in (d1, d2))
    assert d1["means"].pop("FID") == f1 and d2["means"].pop("FID") == f2 and abs(f1 - f2) <= 1e-9 * f1   # (eigh's threads may differ)
    assert d1 == d2
    lines = [ln for ln in out1.splitlines() if " \t " in ln]
    assert lines == [ln for ln in out2.splitlines() if " \t " in ln] and lines[-1].startswith("FID \t ")
