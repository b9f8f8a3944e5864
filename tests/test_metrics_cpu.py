"""CPU-only: the quality metrics (PSNR / SSIM, csrc/metrics.hip) -- the fp64 restatement against the reference's outputs
(tests/golden/metrics.npz), the C ABI's host-only answers, argument checks before any launch, the evaluation aliases, gather_rows, and
the CLI's file discovery."""
import ctypes
import json
import math
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref64 as M
from pixelsynth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ssim_bound_vs_reference(name):
    """SSIM bound against the reference's fp32 outputs: flat regions cancel in its E[x^2] - mu^2 (3e-5 of its own error here); on
    the uint8-quantised pairs its own fp32 error is 1.2e-6 (metrics.npz err32/)."""
    return 2e-4 if M.is_flat(name) else 2e-6 if name.startswith("uint8") else 1e-6


def assert_rows_close(got, want, psnr_tol, ssim_tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.array_equal(np.isinf(got), np.isinf(want)), (what, got, want)
    ok = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        d = np.where(ok, np.abs(got - want), 0.0)
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), what
    assert d[:, :3].max() <= psnr_tol, (what, "psnr", d[:, :3].max())
    assert d[:, 3:].max() <= ssim_tol, (what, "ssim", d[:, 3:].max())
    return d[:, :3].max(), d[:, 3:].max()


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


def test_golden_cases_are_the_listed_ones(golden_dir):
    z = golden(golden_dir)
    assert [tuple(c) for c in json.loads(str(z["cases"]))] == [tuple(c) for c in M.CASES]
    for case in M.CASES:
        a, b, m = M.case_inputs(case)
        s = sum(np.asarray(x, np.float64).sum() for x in (a, b, m) if x is not None)
        assert math.isclose(s, float(z["sum/" + case[0]]), rel_tol=1e-12), case[0]   # the generators still make the same inputs


def test_fp64_restatement_matches_reference(golden_dir):
    z = golden(golden_dir)
    for case in M.CASES:
        a, b, m = M.case_inputs(case)
        assert_rows_close(M.metrics64(a, b, m), z["ref/" + case[0]], 1e-4, ssim_bound_vs_reference(case[0]), case[0])


def test_kernel_window_is_the_references():
    """csrc/metrics.hip holds the fp32 taps of ssim.py's gaussian(11, 1.5), normalised in fp32 as the reference does."""
    src = open(os.path.join(ROOT, "pixelsynth_amd", "csrc", "metrics.hip")).read()
    body = re.search(r"c_gauss\[11\]\s*=\s*\{([^}]*)\}", src).group(1)
    taps = np.array([float.fromhex(t.strip().rstrip("f")) for t in body.split(",")], np.float32)
    g = torch.tensor([math.exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    assert np.array_equal(taps, (g / g.sum()).numpy())
    w2 = M.window2d()
    assert np.array_equal(w2, np.outer(taps, taps).astype(np.float32).astype(np.float64))


def test_workspace_bytes_through_ctypes():
    L = _lib.lib()
    assert L.ps_image_metrics_workspace_bytes(2, 3, 256, 256) == 2 * 64 * 8 * 8
    assert L.ps_image_metrics_workspace_bytes(1, 3, 5, 7) == 64
    assert L.ps_image_metrics_workspace_bytes(3, 1, 33, 65) == 3 * 6 * 64
    assert L.ps_image_metrics_workspace_bytes(0, 3, 8, 8) == 0


def test_entry_point_rejects_bad_arguments_before_launching():
    L = _lib.lib()
    st = (ctypes.c_int64 * 4)(3 * 64, 64, 8, 1)
    fake = ctypes.c_void_p(4096)   # never dereferenced: every check runs before a launch
    ws = L.ps_image_metrics_workspace_bytes(1, 3, 8, 8)

    def call(C=3, dtype=0, B=1, H=8, W=8, wsb=ws, strides=st):
        return L.ps_image_metrics(fake, strides, fake, strides, dtype, None, B, C, H, W, fake, fake, wsb, None)
    for kw, msg in ((dict(C=2), b"C must be 1 or 3"), (dict(dtype=5), b"dtype"), (dict(B=0), b"B"), (dict(H=0), b"H, W"),
                    (dict(wsb=ws - 1), b"workspace"), (dict(strides=(ctypes.c_int64 * 4)(1, 1, -1, 1)), b"negative stride")):
        assert call(**kw) == -1, kw
        assert msg in L.ps_last_error(), (kw, L.ps_last_error())


def test_python_entry_points_check_before_launching():
    from pixelsynth_amd.evaluation import score_views
    from pixelsynth_amd.evaluation.metrics import psnr, ssim_metric
    from pixelsynth_amd.image_metrics import image_metrics
    from pixelsynth_amd.losses.ssim import SSIM, ssim
    a = torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        psnr(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ssim_metric(a, a, mask=torch.ones(2, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        score_views(a, a, torch.zeros(2, 16, 16, dtype=torch.bool))
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        image_metrics(torch.rand(2, 2, 16, 16), torch.rand(2, 2, 16, 16))
    with pytest.raises(ValueError, match="differ in shape"):
        psnr(a, torch.rand(2, 3, 16, 15))
    with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
        psnr(a[0], a[0])
    with pytest.raises(ValueError, match="mask must be"):
        psnr(a, a, torch.ones(2, 3, 16, 16))
    with pytest.raises(TypeError, match="float32 or both uint8"):
        psnr(a.double(), a.double())
    with pytest.raises(NotImplementedError):
        ssim(a, a, window_size=13)
    with pytest.raises(NotImplementedError):
        SSIM(window_size=13)


def test_evaluation_aliases_in_a_fresh_interpreter():
    code = (
        "import sys\n"
        "import pixelsynth_amd.compat as c\n"
        "before = dict(c.ALIASES)\n"
        "assert sorted(c.install_evaluation_aliases()) == ['evaluation.metrics', 'models.losses.ssim']\n"
        "from evaluation.metrics import psnr, ssim_metric, perceptual_sim\n"
        "from models.losses.ssim import ssim, SSIM\n"
        "import pixelsynth_amd.evaluation.metrics as em, pixelsynth_amd.losses.ssim as ls\n"
        "assert psnr is em.psnr and ssim_metric is em.ssim_metric and ssim is ls.ssim and SSIM is ls.SSIM\n"
        "assert c.ALIASES == before and not any(k in sys.modules for k in c.ALIASES)\n"
        "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_gather_rows_single_process():
    from pixelsynth_amd import distributed as D
    rows = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert np.array_equal(D.gather_rows(rows, 4), rows)


def test_gather_rows_across_ranks():
    """gloo, world size 2: rows computed on the dealt items come back in item order on every rank."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "tests", "_gather_rows_worker.py")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def _write_pngs(d, n, size=(12, 10)):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        Image.fromarray(np.full(size + (3,), i, np.uint8)).save(os.path.join(d, f"{i}.png"))


def test_cli_file_discovery(tmp_path):
    from pixelsynth_amd.evaluate import discover
    pred, gt, smp = str(tmp_path / "pred"), str(tmp_path / "gt"), str(tmp_path / "sampled")
    _write_pngs(pred, 5)
    _write_pngs(gt, 6)
    _write_pngs(smp, 3)
    items = discover(pred, gt)
    assert [os.path.basename(p) for p, _, _ in items] == [f"{i}.png" for i in range(5)]
    assert all(g == os.path.join(gt, os.path.basename(p)) and s is None for p, g, s in items)
    assert len(discover(pred, gt, max_img=3)) == 3 and discover(pred, gt, max_img=0) == []
    with pytest.raises(FileNotFoundError, match="missing"):
        discover(pred, gt, max_img=6)          # pred has no 5.png
    with pytest.raises(FileNotFoundError, match="missing"):
        discover(pred, gt, smp)                # sampled stops at 2.png
    items = discover(pred, gt, smp, max_img=3)
    assert [s for _, _, s in items] == [os.path.join(smp, f"{i}.png") for i in range(3)]


def test_cli_decodes_rgb_and_the_sampled_mask(tmp_path):
    from PIL import Image

    from pixelsynth_amd.evaluate import _decode, summarize
    rs = np.random.RandomState(0)
    gt = rs.randint(0, 256, (9, 7, 3)).astype(np.uint8)
    smp = gt.copy()
    smp[2:5, 1, 0] ^= 1                                       # one channel off: not visible
    for name, arr in (("p.png", gt[..., 0]), ("g.png", gt), ("s.png", smp)):
        Image.fromarray(arr).save(str(tmp_path / name))
    p, g, m = _decode((str(tmp_path / "p.png"), str(tmp_path / "g.png"), str(tmp_path / "s.png")))
    assert p.shape == (9, 7, 3) and np.array_equal(p[..., 2], gt[..., 0]) and np.array_equal(g, gt)
    want = np.ones((9, 7), np.float32)
    want[2:5, 1] = 0
    assert m.dtype == np.float32 and np.array_equal(m, want)
    rows = np.array([[np.inf, 30.0, np.inf, 0.5, 0.25, 0.0], [20.0, 150.0, 10.0, 1.0, 0.75, 1.0]])
    s = summarize(rows, masked=True)
    assert list(s) == ["PSNR", "PSNR_invis", "PSNR_vis", "SSIM", "SSIM_invis", "SSIM_vis"]
    assert s["PSNR"] == 60.0 and s["PSNR_vis"] == 65.0 and s["PSNR_invis"] == 55.0 and s["SSIM_vis"] == 0.5
    assert list(summarize(rows, masked=False)) == ["PSNR", "SSIM"]
