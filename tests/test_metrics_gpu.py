"""GPU: the quality-metric kernel (csrc/metrics.hip) against the reference's outputs (tests/golden/metrics.npz) and the fp64
restatement (tests/golden/metrics_ref64.py); bit-level properties (uint8 = fp32 of x / 255, channels-last = contiguous, run to run,
batch position); the edge cases; score_views on rendered views; the CLI on PNG directories, one rank and two."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref64 as M
from pixelsynth_amd import synthetic as syn
from pixelsynth_amd.image_metrics import COLUMNS, image_metrics
from test_metrics_cpu import assert_rows_close, ssim_bound_vs_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
# the kernel forms the moments in fp64: against the fp64 restatement the flat cases need no looser bound than the textured ones
SSIM_VS_FP64 = 1e-6


def run(a, b, m=None):
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return image_metrics(t(a), t(b), t(m)).cpu().numpy()


def test_golden_cases_against_reference_and_fp64(golden_dir):
    z = np.load(os.path.join(golden_dir, "metrics.npz"))
    worst = {"ref_psnr": 0.0, "ref_ssim_textured": 0.0, "ref_ssim_flat": 0.0, "fp64_psnr": 0.0, "fp64_ssim": 0.0}
    for case in M.CASES:
        a, b, m = M.case_inputs(case)
        got = run(a, b, m)
        dp, ds = assert_rows_close(got, z["ref/" + case[0]], 1e-4, ssim_bound_vs_reference(case[0]), case[0])
        worst["ref_psnr"] = max(worst["ref_psnr"], dp)
        key = "ref_ssim_flat" if M.is_flat(case[0]) else "ref_ssim_textured"
        worst[key] = max(worst[key], ds)
        dp, ds = assert_rows_close(got, M.metrics64(a, b, m), 1e-4, SSIM_VS_FP64, case[0])
        worst["fp64_psnr"], worst["fp64_ssim"] = max(worst["fp64_psnr"], dp), max(worst["fp64_ssim"], ds)
    print("metrics error maxima:", json.dumps({k: float("%.3g" % v) for k, v in worst.items()}))


@pytest.mark.parametrize("B,C,H,W", [(128, 3, 24, 40), (7, 1, 33, 65), (3, 3, 70, 31), (2, 3, 1, 1), (5, 3, 64, 64)])
def test_random_shapes_against_fp64(B, C, H, W):
    rs = np.random.RandomState(B * 1000 + H)
    a = rs.rand(B, C, H, W).astype(np.float32)
    b = np.clip(a + rs.randn(B, C, H, W).astype(np.float32) * np.float32(0.1), 0, 1).astype(np.float32)
    m = rs.rand(B, 1, H, W).astype(np.float32)
    assert_rows_close(run(a, b, m), M.metrics64(a, b, m), 1e-4, SSIM_VS_FP64, (B, C, H, W))
    assert_rows_close(run(a, b), M.metrics64(a, b), 1e-4, SSIM_VS_FP64, (B, C, H, W))


def test_uint8_path_is_bit_identical_to_fp32_of_to_tensor():
    a, b = syn.metric_pair(21, 4, 3, 77, 90, "uint8")
    m = syn.metric_mask("fractional", 22, 4, 77, 90)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    fa, fb = ta.float().div(255), tb.float().div(255)        # TF.to_tensor, on the host
    u8 = image_metrics(ta.to(DEV), tb.to(DEV), torch.from_numpy(m).to(DEV)).cpu().numpy()
    f32 = image_metrics(fa.to(DEV), fb.to(DEV), torch.from_numpy(m).to(DEV)).cpu().numpy()
    assert np.array_equal(u8, f32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_channels_last_is_bit_identical(dtype):
    a, b = syn.metric_pair(23, 3, 3, 45, 70, "uint8" if dtype == torch.uint8 else "noise_blur")
    m = torch.from_numpy(syn.metric_mask("ragged", 0, 3, 45, 70)).to(DEV)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    assert not cl(ta).is_contiguous()
    want = image_metrics(ta, tb, m).cpu().numpy()
    assert np.array_equal(image_metrics(cl(ta), cl(tb), m).cpu().numpy(), want)
    nhwc = ta.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # the CLI's upload layout
    assert np.array_equal(image_metrics(nhwc, tb, m).cpu().numpy(), want)


def test_reproducible_and_independent_of_batch_position():
    a, b = syn.metric_pair(31, 128, 3, 64, 64, "noise_blur")
    m = syn.metric_mask("fractional", 32, 128, 64, 64)
    ta, tb, tm = (torch.from_numpy(x).to(DEV) for x in (a, b, m))
    r1 = image_metrics(ta, tb, tm).cpu().numpy()
    r2 = image_metrics(ta, tb, tm).cpu().numpy()
    assert np.array_equal(r1, r2)
    one = image_metrics(ta[5:6], tb[5:6], tm[5:6]).cpu().numpy()[0]
    for pos in (0, 63, 127):
        idx = [i for i in range(128) if i != 5]
        idx.insert(pos, 5)
        idx = torch.tensor(idx, device=DEV)
        r = image_metrics(ta[idx], tb[idx], tm[idx]).cpu().numpy()
        assert np.array_equal(r[pos], one), pos


def test_identical_empty_and_full():
    a, _ = syn.metric_pair(41, 2, 3, 96, 80, "noise_blur")
    B, _, H, W = a.shape
    r = run(a, a, syn.metric_mask("ragged", 0, B, H, W))
    assert np.all(np.isposinf(r[:, [0, 1, 2]])) and np.all(np.abs(r[:, [3, 4, 5]] - 1) <= 1e-7), r
    a, b = syn.metric_pair(42, 2, 3, 96, 80, "noise_blur")
    r = run(a, b, syn.metric_mask("empty", 0, B, H, W))
    assert np.all(np.isposinf(r[:, 1])) and np.all(r[:, 4] == 0), r
    assert np.all(np.isfinite(r[:, 2])) and np.allclose(r[:, 2], r[:, 0], rtol=0, atol=1e-4)
    r = run(a, b, syn.metric_mask("full", 0, B, H, W))
    assert np.allclose(r[:, 1], r[:, 0], rtol=0, atol=1e-4) and np.allclose(r[:, 4], r[:, 3], rtol=0, atol=1e-6), r
    assert np.all(np.isposinf(r[:, 2])) and np.all(r[:, 5] == 0)
    assert np.all(np.isnan(run(a, b)[:, [1, 2, 4, 5]]))


def test_reference_named_entry_points():
    from pixelsynth_amd.evaluation.metrics import perceptual_sim, psnr, ssim_metric
    from pixelsynth_amd.losses.ssim import SSIM, ssim
    a, b = (torch.from_numpy(x).to(DEV) for x in syn.metric_pair(51, 3, 3, 40, 40, "noise_blur"))
    m = torch.from_numpy(syn.metric_mask("ragged", 0, 3, 40, 40)).to(DEV)
    rows = image_metrics(a, b, m)
    assert torch.equal(psnr(a, b), image_metrics(a, b)[:, 0]) and torch.equal(psnr(a, b, m), rows[:, 1])
    assert torch.equal(ssim_metric(a, b), rows[:, 3]) and torch.equal(ssim_metric(a, b, 1 - m), rows[:, 5])
    assert ssim(a, b).dim() == 0 and torch.allclose(ssim(a, b), rows[:, 3].mean())
    assert torch.equal(ssim(a, b, mask=m), rows[:, 4])               # masked: the vector even with size_average (ssim.py:61-67)
    assert torch.equal(SSIM()(a, b, m), rows[:, 4]) and torch.equal(SSIM(size_average=False)(a, b), rows[:, 3])
    net = lambda x, y: (x - y).abs().mean((1, 2, 3))
    assert torch.equal(perceptual_sim(a, b, net), net(a * 2 - 1, b * 2 - 1))


def test_score_views_on_synthesized_views():
    import types

    sys.path.insert(0, ROOT)
    import bench
    from pixelsynth_amd.evaluation import score_views
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts
    o = vars(bench.make_opts()).copy()
    o.update(vars(syn.network_opts()))
    o.update(vqvae=True, min_z=0.5, max_z=10.0)
    model = ZbufferModelPts(types.SimpleNamespace(**o)).eval()
    model.outpaint2.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()})
    model.vqvae.load_state_dict({k: torch.from_numpy(v) for k, v in syn.vqvae_state_dict(0).items()})
    for mod in (model.pts_regressor, model.projector):
        shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, 5).items()})
    model = model.to(DEV)
    V = 4
    d, host = bench.make_inputs(0, V, DEV, cameras="mp3d")
    src = d["img"][:1].contiguous()
    out = model.synthesize_views(src, torch.zeros(V, dtype=torch.long, device=DEV), d["K"], d["Kinv"], d["P"], d["Pinv"], d["RT2"],
                                 d["RT2inv"], temperature=0.7, uniforms=d["uniforms"])
    pred, bg = out["PredImg"], out["background_mask"]
    gt = src.expand(V, -1, -1, -1)
    assert bg.dtype == torch.bool and 0 < int(bg.sum()) < bg.numel()
    s = score_views(pred, gt, bg)
    assert sorted(s) == sorted(COLUMNS) and all(v.shape == (V,) for v in s.values())
    p, g = (pred * 0.5 + 0.5).cpu().numpy(), (gt * 0.5 + 0.5).cpu().numpy()
    vis = (~bg).float()[:, None].cpu().numpy()
    want = M.metrics64(p, g, vis)
    got = np.stack([s[c].cpu().numpy() for c in COLUMNS], 1)
    assert_rows_close(got, want, 1e-4, SSIM_VS_FP64, "score_views")
    s2 = score_views(pred, gt)
    assert sorted(s2) == ["psnr", "ssim"] and torch.equal(s2["psnr"], s["psnr"])


def _png_dirs(tmp_path, n=11, H=40, W=56):
    from PIL import Image
    a, b = syn.metric_pair(61, n, 3, H, W, "uint8")
    smp = b.copy()
    smp[:, :, :, W // 2:] = 0                                              # the right half "outpainted"
    dirs = {k: str(tmp_path / k) for k in ("pred", "gt", "sampled")}
    for k, arr in (("pred", a), ("gt", b), ("sampled", smp)):
        os.makedirs(dirs[k])
        for i in range(n):
            Image.fromarray(np.ascontiguousarray(arr[i].transpose(1, 2, 0))).save(os.path.join(dirs[k], f"{i}.png"))
    mask = np.all(b == smp, axis=1, keepdims=True).astype(np.float32)
    return dirs, a, b, mask


def _cli(args, env=None, nproc=1):
    if nproc == 1:
        cmd = [sys.executable, "-m", "pixelsynth_amd.evaluate"] + args
    else:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
               "127.0.0.1", "--master-port", str(port), "-m", "pixelsynth_amd.evaluate"] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


@pytest.mark.parametrize("sampled", [False, True])
def test_cli_end_to_end(tmp_path, sampled):
    from pixelsynth_amd.evaluate import summarize
    dirs, a, b, mask = _png_dirs(tmp_path)
    js = str(tmp_path / "out.json")
    args = ["--pred", dirs["pred"], "--gt", dirs["gt"], "--batch", "4", "--json", js] + (["--sampled", dirs["sampled"]] if sampled else [])
    stdout = _cli(args)
    rows = image_metrics(torch.from_numpy(b).to(DEV), torch.from_numpy(a).to(DEV),
                         torch.from_numpy(mask).to(DEV) if sampled else None).cpu().double().numpy()
    means = summarize(rows, sampled)
    lines = [ln for ln in stdout.splitlines() if " \t " in ln]
    assert lines == ["%s \t %0.5f" % (k, v) for k, v in means.items()], stdout
    doc = json.load(open(js))
    cols = COLUMNS if sampled else ("psnr", "ssim")
    assert doc["n"] == len(rows) and doc["means"] == means
    assert [[r[c] for c in cols] for r in doc["rows"]] == [[float(rows[i, COLUMNS.index(c)]) for c in cols] for i in range(len(rows))]
    assert [r["index"] for r in doc["rows"]] == list(range(len(rows)))
    sub = _cli(args[:-2] + ["--max-img", "5"] + (["--sampled", dirs["sampled"]] if sampled else []))
    assert [ln for ln in sub.splitlines() if " \t " in ln] == ["%s \t %0.5f" % kv for kv in summarize(rows[:5], sampled).items()]


def test_cli_two_ranks_equal_one(tmp_path):
    dirs, _, _, _ = _png_dirs(tmp_path)
    base = ["--pred", dirs["pred"], "--gt", dirs["gt"], "--sampled", dirs["sampled"], "--batch", "2"]
    one, two = str(tmp_path / "one.json"), str(tmp_path / "two.json")
    out1 = _cli(base + ["--json", one])
    out2 = _cli(base + ["--json", two], env={"PS_DRYRUN_ONE_GPU": "1"}, nproc=2)
    assert json.load(open(one)) == json.load(open(two))
    assert [ln for ln in out1.splitlines() if " \t " in ln] == [ln for ln in out2.splitlines() if " \t " in ln]
