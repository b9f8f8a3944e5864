"""Generate tests/golden/fid.npz from the fp64 restatement (fid_ref64.py).  pytorch_fid and torchvision are imported if they are there
(then their InceptionV3 / Inception3 gives the key list, "source" says which); neither was where this file was last written, so the
key list comes from pixelsynth_amd.networks.inception and is marked "source": "restated".  The file holds the cases, a checksum of every
case's input, the fp64 features, err32 = max |fp32 run - fp64 run| of the restatement per case, and for the two 64-image sets of the
FID test the fp64 FID, the FID of the restatement's fp32 features and their relative difference.  No weights, no images.

    python tests/golden/make_fid_golden.py
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

import fid_ref64 as R  # noqa: E402


def state_keys():
    """-> (source, [[key, shape], ...]) of the trunk (no fc.*, AuxLogits.*, num_batches_tracked)"""
    skip = lambda k: k.startswith(("fc.", "AuxLogits.")) or k.endswith("num_batches_tracked")
    try:
        from torchvision.models import inception_v3
        net, source = inception_v3(weights=None, aux_logits=False, init_weights=False), "torchvision"
    except ImportError:
        from pixelsynth_amd.networks.inception import FIDInception
        net, source = FIDInception(), "restated"
    return source, [[k, list(v.shape)] for k, v in net.state_dict().items() if not skip(k)]


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = R.weights()
    source, keys = state_keys()
    out = {"cases": np.array(json.dumps(R.CASES)), "weight_seed": np.array(R.WEIGHT_SEED), "source": np.array(source),
           "state_keys": np.array(json.dumps(keys)), "fid_sets": np.array(json.dumps(R.FID_SETS))}
    with torch.no_grad():
        for case in R.CASES:
            x = R.case_input(case)
            f64 = R.features(sd, x, torch.float64).numpy()
            f32 = R.features(sd, x, torch.float32).numpy().astype(np.float64)
            out["sum/" + case[0]] = np.array(float(np.asarray(x, np.float64).sum()))
            out["f64/" + case[0]] = f64
            out["err32/" + case[0]] = np.array(np.abs(f32 - f64).max())
            print(f"{case[0]:10s} fp32 vs fp64: {out['err32/' + case[0]]:.3e}  features: mean {f64.mean():.3f} max {f64.max():.3f} "
                  f"zero {np.mean(f64 == 0):.3f}", flush=True)
        sets = R.fid_sets()
        rows = {}
        for dt in (torch.float64, torch.float32):
            rows[dt] = [np.concatenate([R.features(sd, s[i:i + 16], dt).numpy() for i in range(0, len(s), 16)]) for s in sets]
        fid64, fid32 = R.fid64(*rows[torch.float64]), R.fid64(*rows[torch.float32])
        out["fid/sum"] = np.array([float(np.asarray(s, np.float64).sum()) for s in sets])
        out["fid/fid64"], out["fid/fid32"] = np.array(fid64), np.array(fid32)
        out["fid/rel32"] = np.array(abs(fid32 - fid64) / fid64)
        out["fid/row_err32"] = np.array(max(np.abs(a - b).max() for a, b in zip(rows[torch.float64], rows[torch.float32])))
        print(f"FID of the two sets: fp64 {fid64:.9f}  fp32 features {fid32:.9f}  relative {out['fid/rel32']:.3e}  "
              f"rows fp32 vs fp64 {out['fid/row_err32']:.3e}", flush=True)
    np.savez_compressed(os.path.join(HERE, "fid.npz"), **out)


if __name__ == "__main__":
    main()
