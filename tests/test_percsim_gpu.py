"""GPU: PercSim on the HIP path (csrc/percsim.hip around the split-fp16 convolutions) against the reference's outputs
(tests/golden/percsim.npz) and the fp64 restatement (tests/golden/percsim_ref64.py), per tap and in total; the torch path outside the
HIP shapes; bit-level properties (run to run, batch position and size, uint8 = fp32 of x / 255, channels-last = contiguous, vis = the
explicitly masked images); the overflow guard; a NaN or +inf pixel, or a NaN in the mask, gives its own pair's score NaN with the
guard's warning and leaves the others to the torch formula; score_views; the CLI with --vgg16 on one rank and two.  The three passes
of csrc/percsim.hip on their own: tests/test_percsim_passes_gpu.py."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import percsim_ref64 as R
from pixelsynth_amd import synthetic as syn
from pixelsynth_amd.networks import f16x3
from pixelsynth_amd.networks.pretrained_networks import PNet
from pixelsynth_amd.perceptual import COLUMNS, perceptual_rows
from test_metrics_gpu import _cli, _png_dirs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# Measured maxima on the MI355X (printed by the first test): against fp64 8.2e-8 per tap and 1.7e-7 in total, against the reference
# 1.2e-7 and 2.4e-7; the bounds are about four times those.
BOUND_TAP, BOUND_TOTAL = 4e-7, 8e-7


@pytest.fixture(scope="module")
def pnet():
    torch.cuda.set_device(DEV)
    sd = {k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(R.WEIGHT_SEED).items()}
    return PNet(use_gpu=True, weights=sd)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def forward_rows(net, x0, x1):
    """(B, 6): the five per-tap scores and the total of PNet.forward on images in [0, 1]"""
    with torch.no_grad():
        val, layers = net(t(x0) * 2 - 1, t(x1) * 2 - 1, retPerLayer=True)
    return torch.cat([torch.stack(layers, 1), val[:, None]], 1).cpu().double().numpy()


def test_golden_cases_against_reference_and_fp64(pnet, golden_dir):
    z = np.load(os.path.join(golden_dir, "percsim.npz"))
    worst = {"ref_tap": 0.0, "ref_total": 0.0, "fp64_tap": 0.0, "fp64_total": 0.0}
    for case in R.CASES:
        a, b, m = R.case_inputs(case)
        got = np.stack([forward_rows(pnet, x0, x1) for x0, x1 in R.variants(a, b, m)])
        rows = perceptual_rows(pnet, t(a), t(b), None if m is None else t(m)).cpu().double().numpy()
        if case[3] % 256 == 0 and case[4] % 256 == 0:                     # the same HIP pass: the same bits
            assert np.array_equal(rows[:, :got.shape[0]].T, got[:, :, 5]), case[0]
        ref, r64, err32 = z["ref/" + case[0]].astype(np.float64), R.case64(case), z["err32/" + case[0]]
        for key, want, extra in (("ref", ref, err32), ("fp64", r64, 0.0)):
            d = np.abs(got - want).max((0, 1))
            assert (d[:5] <= BOUND_TAP + extra[:5] if key == "ref" else d[:5] <= BOUND_TAP).all(), (case[0], key, d)
            assert d[5] <= BOUND_TOTAL + (extra[5] if key == "ref" else 0.0), (case[0], key, d)
            worst[key + "_tap"] = max(worst[key + "_tap"], float(d[:5].max()))
            worst[key + "_total"] = max(worst[key + "_total"], float(d[5]))
    print("percsim error maxima:", json.dumps({k: float("%.3g" % v) for k, v in worst.items()}))


def test_outside_the_hip_shapes_is_the_torch_formula(pnet):
    a, b = syn.metric_pair(31, 2, 3, 96, 160)
    x0, x1 = t(a) * 2 - 1, t(b) * 2 - 1
    assert not pnet.hip_takes(x0, x1)
    with torch.no_grad():
        want = pnet.torch_forward(x0, x1)
    # the same torch formula (MIOpen may pick another algorithm from call to call: not bit for bit)
    torch.testing.assert_close(pnet(x0, x1), want, rtol=0, atol=1e-6)
    torch.testing.assert_close(perceptual_rows(pnet, t(a), t(b))[:, 0], want, rtol=0, atol=1e-6)


def test_bit_level_properties(pnet):
    a, b = syn.metric_pair(32, 3, 3, 256, 256)
    m = syn.metric_mask("ragged", 33, 3, 256, 256)
    one = perceptual_rows(pnet, t(a), t(b), t(m))
    assert torch.equal(one, perceptual_rows(pnet, t(a), t(b), t(m))), "run to run"
    for lo, hi in ((1, 2), (1, 3), (0, 2), (2, 3)):
        part = perceptual_rows(pnet, t(a[lo:hi]), t(b[lo:hi]), t(m[lo:hi]))
        assert torch.equal(part, one[lo:hi]), (lo, hi)
    nhwc = lambda x: t(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
    assert torch.equal(perceptual_rows(pnet, nhwc(a), nhwc(b), t(m)), one), "channels-last storage"
    vis = perceptual_rows(pnet, t(a) * t(m), t(b) * t(m))
    inv = perceptual_rows(pnet, t(a) * (1 - t(m)), t(b) * (1 - t(m)))
    assert torch.equal(vis[:, 0], one[:, 1]) and torch.equal(inv[:, 0], one[:, 2])
    assert torch.isnan(perceptual_rows(pnet, t(a), t(b))[:, 1:]).all()


def test_uint8_is_bit_identical_to_fp32_of_to_tensor(pnet):
    a, b = syn.metric_pair(34, 2, 3, 256, 256, "uint8")
    m = syn.metric_mask("fractional", 35, 2, 256, 256)
    fa, fb = torch.from_numpy(a).float().div(255), torch.from_numpy(b).float().div(255)    # TF.to_tensor, on the host
    assert torch.equal(perceptual_rows(pnet, t(a), t(b), t(m)), perceptual_rows(pnet, fa.to(DEV), fb.to(DEV), t(m)))


def test_overflow_guard_reruns_in_fp32(pnet):
    sd = {k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(R.WEIGHT_SEED).items()}
    sd["features.0.weight"] = sd["features.0.weight"] * 3.0e4       # conv1_1's outputs reach past fp16's range
    hot = PNet(use_gpu=True, weights=sd)
    a, b = syn.metric_pair(36, 2, 3, 256, 256)
    x0, x1 = t(a) * 2 - 1, t(b) * 2 - 1
    assert hot.hip_takes(x0, x1)
    with pytest.warns(UserWarning, match="fp16's range"):
        got = hot(x0, x1)
    with torch.no_grad():
        want = hot.torch_forward(x0, x1)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-7)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pnet(t(a) * 2 - 1, t(b) * 2 - 1)                              # the normal weights: no warning
    with f16x3.decoder_conv("fp32"):
        assert not pnet.hip_takes(x0, x1)


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_pixel_gives_its_pair_nan_with_the_warning(pnet, value):
    a, b = syn.metric_pair(39, 2, 3, 256, 256)
    a = a.copy()
    a[1, 1, 100, 37] = value
    x0, x1 = t(a) * 2 - 1, t(b) * 2 - 1
    assert pnet.hip_takes(x0, x1)
    with torch.no_grad():
        want = pnet.torch_forward(x0, x1)
    assert bool(want[1].isnan()) and bool(want[0].isfinite()), "the torch formula"
    with pytest.warns(UserWarning, match="fp16's range"):
        rows = perceptual_rows(pnet, t(a), t(b))
    with pytest.warns(UserWarning, match="fp16's range"):
        got = pnet(x0, x1)
    for mine in (rows[:, 0], got):
        assert bool(mine[1].isnan()), "a pair with a broken pixel must not come out as a clean number"
        torch.testing.assert_close(mine[:1], want[:1], rtol=0, atol=1e-6)
    assert bool(rows[:, 1:].isnan().all())


def test_a_nan_in_the_mask_reaches_vis_and_invis_alone(pnet):
    a, b = syn.metric_pair(40, 2, 3, 256, 256)
    m = syn.metric_mask("fractional", 41, 2, 256, 256).copy()
    clean = perceptual_rows(pnet, t(a), t(b), t(m))
    assert bool(clean.isfinite().all())
    m[1, 0, 9, 200] = float("nan")
    with pytest.warns(UserWarning, match="fp16's range"):
        rows = perceptual_rows(pnet, t(a), t(b), t(m))
    assert bool(rows[1, 1:].isnan().all()), "vis and invis of the image whose mask holds the NaN"
    keep = torch.tensor([[True, True, True], [True, False, False]], device=rows.device)
    assert torch.equal(rows.isfinite(), keep)
    torch.testing.assert_close(rows[keep], clean[keep], rtol=0, atol=1e-6)          # (the rerun is the torch formula)


def test_score_views_columns_match_direct_calls(pnet):
    from pixelsynth_amd.evaluation import score_views
    a, b = syn.metric_pair(37, 2, 3, 256, 256)
    pred, gt = t(a) * 2 - 1, t(b) * 2 - 1
    bg = t(syn.metric_mask("ragged", 38, 2, 256, 256)[:, 0] < 0.5)
    plain = score_views(pred, gt)
    assert set(plain) == {"psnr", "ssim"}
    out = score_views(pred, gt, bg, pnet=pnet)
    direct = perceptual_rows(pnet, pred * 0.5 + 0.5, gt * 0.5 + 0.5, (~bg).unsqueeze(1))
    for k in COLUMNS:
        assert torch.equal(out[k], direct[:, COLUMNS.index(k)]), k
    assert torch.equal(out["psnr"], score_views(pred, gt, bg)["psnr"])
    out1 = score_views(pred, gt, pnet=pnet)
    assert set(out1) == {"psnr", "ssim", "percsim"} and torch.equal(out1["percsim"], direct[:, 0])


@pytest.fixture(scope="module")
def vgg_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vgg") / "vgg16-397923af.pth")
    torch.save({k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(R.WEIGHT_SEED).items()}, path)
    return path


@pytest.mark.parametrize("sampled", [False, True])
def test_cli_percsim_lines(tmp_path, vgg_file, pnet, sampled):
    from pixelsynth_amd.evaluate import ALL_COLUMNS, summarize
    dirs, a, b, mask = _png_dirs(tmp_path, n=3, H=256, W=256)
    js = str(tmp_path / "out.json")
    args = ["--pred", dirs["pred"], "--gt", dirs["gt"], "--batch", "2", "--json", js, "--vgg16", vgg_file]
    stdout = _cli(args + (["--sampled", dirs["sampled"]] if sampled else []))
    lines = [ln for ln in stdout.splitlines() if " \t " in ln]
    names = ["PSNR", "PSNR_invis", "PSNR_vis", "SSIM", "SSIM_invis", "SSIM_vis", "PercSim", "PercSim_invis", "PercSim_vis"]
    assert [ln.split(" \t ")[0] for ln in lines] == (names if sampled else ["PSNR", "SSIM", "PercSim"])
    from pixelsynth_amd.image_metrics import image_metrics
    m = t(mask) if sampled else None
    rows = torch.cat([image_metrics(t(b), t(a), m), perceptual_rows(pnet, t(b), t(a), m)], 1).cpu().double().numpy()
    means = summarize(rows, sampled, True)
    assert lines == ["%s \t %0.5f" % (k, v) for k, v in means.items()], stdout
    doc = json.load(open(js))
    keys = (["psnr", "psnr_vis", "psnr_invis", "ssim", "ssim_vis", "ssim_invis", "percsim", "percsim_vis", "percsim_invis"] if sampled
            else ["psnr", "ssim", "percsim"])
    assert list(doc["means"]) == list(means) and list(doc["rows"][0]) == ["index"] + keys
    for i, row in enumerate(doc["rows"]):
        for k in keys:
            assert row[k] == float(rows[i, ALL_COLUMNS.index(k)]) or (np.isnan(row[k]) and np.isnan(rows[i, ALL_COLUMNS.index(k)])), k


def test_cli_percsim_two_ranks_equal_one(tmp_path, vgg_file):
    dirs, _, _, _ = _png_dirs(tmp_path, n=3, H=256, W=256)
    base = ["--pred", dirs["pred"], "--gt", dirs["gt"], "--sampled", dirs["sampled"], "--batch", "1", "--vgg16", vgg_file]
    one, two = str(tmp_path / "one.json"), str(tmp_path / "two.json")
    out1 = _cli(base + ["--json", one])
    out2 = _cli(base + ["--json", two], env={"PS_DRYRUN_ONE_GPU": "1"}, nproc=2)
    assert json.load(open(one)) == json.load(open(two))
    assert [ln for ln in out1.splitlines() if " \t " in ln] == [ln for ln in out2.splitlines() if " \t " in ln]
