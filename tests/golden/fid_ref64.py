"""A functional restatement of the FID network (Inception-v3 as pytorch_fid runs it, dims = 2048), written from the layer table of its
specification and from the state dict, without the module's code: plain torch functional calls in the dtype asked for (fp64, the pin;
fp32, whose distance from the fp64 run is what fp32 arithmetic costs on this network -- the yardstick of every float bound of the FID
tests).  pytorch_fid is not importable where this was written, so the architecture is restated, not pinned.

features(sd, x, dtype) -> (N, 2048): sd the state dict (numpy arrays or tensors, torchvision's keys), x (N, 3, H, W) float images in
[0, 1] (numpy).  CASES are the golden cases of tests/golden/fid.npz; fid_sets() the two image sets of the FID test."""
import numpy as np
import torch
import torch.nn.functional as F

from pixelsynth_amd import synthetic as syn

WEIGHT_SEED = 11
# (name, kind, seed, H, W): "noise" U(0, 1) pixels, "blur" their 3 x 3 box blur
CASES = [["noise299", "noise", 71, 299, 299], ["blur299", "blur", 72, 299, 299], ["blur256", "blur", 73, 256, 256]]
FID_SETS = {"n": 64, "size": 256, "seeds": [81, 82]}


def case_input(case):
    _, kind, seed, H, W = case
    a, b = syn.metric_pair(seed, 1, 3, H, W)
    return a if kind == "noise" else b


def fid_sets():
    """-> two (64, 3, 256, 256) float32 image sets in [0, 1]: synthetic.image of two seeds"""
    return [syn.image(s, FID_SETS["n"], 3, FID_SETS["size"]) * np.float32(0.5) + np.float32(0.5) for s in FID_SETS["seeds"]]


def weights(seed=WEIGHT_SEED):
    return syn.inception_state_dict(seed)


def features(sd, x, dtype=torch.float64, device="cpu"):
    t = lambda v: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(device=device, dtype=dtype)

    def cbr(h, name, stride=1, padding=0):
        w, g, b = t(sd[name + ".conv.weight"]), t(sd[name + ".bn.weight"]), t(sd[name + ".bn.bias"])
        m, v = t(sd[name + ".bn.running_mean"]), t(sd[name + ".bn.running_var"])
        y = F.conv2d(h, w, None, stride, padding)
        y = (y - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + 0.001) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        return torch.relu(y)

    avg = lambda h: F.avg_pool2d(h, 3, 1, 1, count_include_pad=False)
    x = t(x)
    if x.shape[2] != 299 or x.shape[3] != 299:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    x = 2 * x - 1
    x = cbr(x, "Conv2d_1a_3x3", 2)
    x = cbr(x, "Conv2d_2a_3x3")
    x = cbr(x, "Conv2d_2b_3x3", 1, 1)
    x = F.max_pool2d(x, 3, 2)
    x = cbr(x, "Conv2d_3b_1x1")
    x = cbr(x, "Conv2d_4a_3x3")
    x = F.max_pool2d(x, 3, 2)
    for blk in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        p = blk + "."
        b1 = cbr(x, p + "branch1x1")
        b5 = cbr(cbr(x, p + "branch5x5_1"), p + "branch5x5_2", 1, 2)
        b3 = cbr(cbr(cbr(x, p + "branch3x3dbl_1"), p + "branch3x3dbl_2", 1, 1), p + "branch3x3dbl_3", 1, 1)
        bp = cbr(avg(x), p + "branch_pool")
        x = torch.cat([b1, b5, b3, bp], 1)
    b3 = cbr(x, "Mixed_6a.branch3x3", 2)
    bd = cbr(cbr(cbr(x, "Mixed_6a.branch3x3dbl_1"), "Mixed_6a.branch3x3dbl_2", 1, 1), "Mixed_6a.branch3x3dbl_3", 2)
    x = torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)
    row, col = (0, 3), (3, 0)             # the padding of a (1, 7) and of a (7, 1) kernel
    for blk in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        p = blk + "."
        b1 = cbr(x, p + "branch1x1")
        b7 = cbr(cbr(cbr(x, p + "branch7x7_1"), p + "branch7x7_2", 1, row), p + "branch7x7_3", 1, col)
        bd = cbr(x, p + "branch7x7dbl_1")
        bd = cbr(cbr(bd, p + "branch7x7dbl_2", 1, col), p + "branch7x7dbl_3", 1, row)
        bd = cbr(cbr(bd, p + "branch7x7dbl_4", 1, col), p + "branch7x7dbl_5", 1, row)
        bp = cbr(avg(x), p + "branch_pool")
        x = torch.cat([b1, b7, bd, bp], 1)
    b3 = cbr(cbr(x, "Mixed_7a.branch3x3_1"), "Mixed_7a.branch3x3_2", 2)
    b7 = cbr(cbr(cbr(x, "Mixed_7a.branch7x7x3_1"), "Mixed_7a.branch7x7x3_2", 1, row), "Mixed_7a.branch7x7x3_3", 1, col)
    b7 = cbr(b7, "Mixed_7a.branch7x7x3_4", 2)
    x = torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)
    for blk, pool in (("Mixed_7b", avg), ("Mixed_7c", lambda h: F.max_pool2d(h, 3, 1, 1))):
        p = blk + "."
        b1 = cbr(x, p + "branch1x1")
        b3 = cbr(x, p + "branch3x3_1")
        b3 = torch.cat([cbr(b3, p + "branch3x3_2a", 1, (0, 1)), cbr(b3, p + "branch3x3_2b", 1, (1, 0))], 1)
        bd = cbr(cbr(x, p + "branch3x3dbl_1"), p + "branch3x3dbl_2", 1, 1)
        bd = torch.cat([cbr(bd, p + "branch3x3dbl_3a", 1, (0, 1)), cbr(bd, p + "branch3x3dbl_3b", 1, (1, 0))], 1)
        bp = cbr(pool(x), p + "branch_pool")
        x = torch.cat([b1, b3, bd, bp], 1)
    return x.mean((2, 3))


def fid64(rows1, rows2):
    """FID of two sets of rows in numpy fp64, the same definition as pixelsynth_amd.fid.frechet_distance written independently"""
    out = []
    for r in (rows1, rows2):
        r = np.asarray(r, np.float64)
        out.append((r.mean(0), np.cov(r, rowvar=False)))
    (m1, s1), (m2, s2) = out
    w, v = np.linalg.eigh(s1)
    root = (v * np.sqrt(np.maximum(w, 0))) @ v.T
    m = root @ s2 @ root
    ev = np.maximum(np.linalg.eigvalsh((m + m.T) / 2), 0)
    return float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(ev).sum())
