"""Generate tests/golden/metrics.npz by IMPORTING the reference's evaluation/metrics.py (read-only; it needs torch alone) and running it
on the CPU in fp32.  The file holds the cases (metrics_ref64.CASES: the seeds of pixelsynth_amd/synthetic.py's generators), a checksum
of every case's inputs, the reference's outputs, and per column how far those are from the fp64 restatement (metrics_ref64.metrics64):
the reference's own fp32 error.  Nothing of the reference is copied.

    python tests/golden/make_metrics_golden.py /path/to/reference
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import metrics_ref64 as M  # noqa: E402


def checksum(*arrays):
    return float(sum(np.asarray(a, np.float64).sum() for a in arrays if a is not None))


def reference_rows(metrics, img1, img2, mask):
    a, b = (torch.from_numpy(x).float().div(255) if x.dtype == np.uint8 else torch.from_numpy(x) for x in (img1, img2))
    rows = np.full((a.shape[0], 6), np.nan, np.float32)
    rows[:, 0] = metrics.psnr(a, b).numpy()
    rows[:, 3] = metrics.ssim_metric(a, b).numpy()
    if mask is not None:
        m = torch.from_numpy(mask)
        for col, mm in ((1, m), (2, 1 - m)):   # calc_errors_quality.py:28-35: invis = 1 - mask
            rows[:, col] = metrics.psnr(a, b, mm).numpy()
            rows[:, col + 3] = metrics.ssim_metric(a, b, mm).numpy()
    return rows


def main(ref_root):
    sys.path.insert(0, ref_root)
    from evaluation import metrics
    out = {"cases": np.array(json.dumps(M.CASES))}
    for case in M.CASES:
        img1, img2, mask = M.case_inputs(case)
        rows = reference_rows(metrics, img1, img2, mask)
        out["ref/" + case[0]] = rows
        out["sum/" + case[0]] = np.array(checksum(img1, img2, mask))
        r64 = M.metrics64(img1, img2, mask)
        with np.errstate(invalid="ignore"):
            d = np.abs(rows.astype(np.float64) - r64)
        d[np.isnan(d)] = 0   # inf - inf, nan columns
        out["err32/" + case[0]] = d.max(0)   # the reference's own fp32 error per column (against fp64), a part of the tests' bounds
        print(f"{case[0]:28s} fp32 reference vs fp64: psnr {d[:, :3].max():.2e} dB  ssim {d[:, 3:].max():.2e}")
    np.savez_compressed(os.path.join(HERE, "metrics.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PIXELSYNTH_REFERENCE", "../pixelsynth"))
