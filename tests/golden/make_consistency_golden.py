"""Generate tests/golden/consistency.npz from the fp64 restatement (consistency_ref64.py): per case a checksum of its inputs, the two
fitted homographies of every item (pixelsynth_amd.consistency.fit_points on the raw points) and the fp64 PSNR_vis per direction.
OpenCV is not needed: the file pins the host fit and the restatement against later change.  Images are not stored; the cases are
rebuilt from their seeds (synthetic.py images, rotations K R K^-1, exact and noisy points, masks).

    python tests/golden/make_consistency_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import consistency_ref64 as R  # noqa: E402


def checksum(z):
    return float(sum(np.asarray(z[k], np.float64).sum() for k in ("view1", "view2", "mask1", "mask2", "reproj1", "reproj2")))


def main():
    out = {"cases": np.array(json.dumps(R.CASES))}
    for case in R.CASES:
        z = R.case_inputs(case)
        H12, H21, psnr = R.case64(case, z)
        out["sum/" + case[0]] = np.array(checksum(z))
        out["H12/" + case[0]], out["H21/" + case[0]], out["psnr64/" + case[0]] = H12, H21, psnr
        print(f"{case[0]:12s} psnr64 {psnr.ravel().round(3).tolist()}", flush=True)
    np.savez_compressed(os.path.join(HERE, "consistency.npz"), **out)


if __name__ == "__main__":
    main()
