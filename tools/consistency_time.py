"""Time the homography consistency kernel (csrc/consistency.hip) on 128 view pairs of 256 x 256 with 0/255 masks, uint8, next to the
same formula in torch ops on the same GPU (the fixed-point source position in fp64, the four taps by index, the fp32 bilinear sum,
the masked comparison and the sums), and check both give the same PSNR_vis.  Also times the CLI's host fit of the homographies.

    python tools/consistency_time.py [--items 128] [--iters 50]

Prints microseconds per batch (_measure.looped_ms: one pair of device events around ITERS calls, after 5 warm-up calls) as one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import consistency_ref64 as R  # noqa: E402
from pixelsynth_amd import consistency as C  # noqa: E402
from _measure import looped_ms  # noqa: E402

S = R.S


def torch_formula(v1, v2, m1, m2, maps):
    """(B, 2) PSNR_vis, clamped, in torch ops: v (B, 3, S, S) uint8, m (B, 1, S, S) uint8, maps (B, 2, 9) fp64"""
    B = v1.shape[0]
    dev = v1.device
    y = torch.arange(S, device=dev, dtype=torch.float64).view(1, S, 1)
    x = torch.arange(S, device=dev, dtype=torch.float64).view(1, 1, S)
    xb = torch.div(x, 64, rounding_mode="floor") * 64
    x1 = x - xb
    out = []
    for k, (src, ref, m) in enumerate(((v2, v1, m1), (v1, v2, m2))):
        M = [maps[:, k, i].view(B, 1, 1) for i in range(9)]
        X0, Y0, W0 = M[0] * xb + M[1] * y + M[2], M[3] * xb + M[4] * y + M[5], M[6] * xb + M[7] * y + M[8]
        Wd = W0 + M[6] * x1
        Wd = torch.where(Wd != 0, 32.0 / torch.where(Wd != 0, Wd, torch.ones_like(Wd)), torch.zeros_like(Wd))
        rnd = lambda v: torch.round(v.nan_to_num(nan=2 ** 31 - 1).clamp(-2 ** 31, 2 ** 31 - 1)).long()
        X, Y = rnd((X0 + M[0] * x1) * Wd), rnd((Y0 + M[3] * x1) * Wd)
        sx, sy = (X >> 5).clamp(-32768, 32767), (Y >> 5).clamp(-32768, 32767)
        fx, fy = (X & 31).float() / 32, (Y & 31).float() / 32
        w = ((1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx)
        tr = (src.float() / 255.0 * 255.0).flip(1)                           # BGR
        flat = tr.reshape(B, 3, S * S)
        warped = 0
        for t_, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            X_, Y_ = sx + dx, sy + dy
            ok = (X_ >= 0) & (X_ < S) & (Y_ >= 0) & (Y_ < S)
            idx = (Y_.clamp(0, S - 1) * S + X_.clamp(0, S - 1)).view(B, 1, -1).expand(B, 3, -1)
            v = torch.gather(flat, 2, idx).view(B, 3, S, S) * ok.unsqueeze(1)
            warped = warped + v * w[t_].unsqueeze(1)
        mf = m.float() / 255.0
        a = warped * mf / 255.0
        b = (mf * (ref.float() / 255.0).flip(1)) * 255.0 / 255.0
        num = ((a - b).pow(2).sum(1, keepdim=True).double() * mf.double()).view(B, -1).sum(1)
        den = 3.0 * mf.double().view(B, -1).sum(1).clamp(min=1)
        out.append((10 * torch.log10(1.0 / (num / den))).float().clamp(max=100))
    return torch.stack(out, 1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B = args.items
    case = ("time", 3, 8, (3.0, -2.0, 1.0), 0.5, "valid")
    z = R.case_inputs(case)
    reps = (B + 7) // 8
    rep = lambda a: np.concatenate([a] * reps)[:B]
    v1, v2, m1, m2 = (torch.from_numpy(rep(z[k])).to(dev) for k in ("view1", "view2", "mask1", "mask2"))
    t0 = time.perf_counter()
    H12, H21 = C.fit_points(list(rep(z["reproj1"])), list(rep(z["reproj2"])))
    t_fit = (time.perf_counter() - t0) * 1e6
    maps_np = C._maps(B, H12, H21, None)
    maps = torch.from_numpy(maps_np).to(dev)
    nbytes = C._lib.call("ps_consistency_workspace_bytes", B, S, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    psnr = torch.empty(B, 2, dtype=torch.float32, device=dev)
    strides = C._images.strides

    def kernel():
        C._lib.call("ps_consistency", v1, strides(v1), v2, strides(v2), 1, m1, m2, 1, maps, B, S, S, 0, None, psnr, ws, nbytes)
    t_kernel = looped_ms(kernel, args.iters, 5) * 1e3
    pin = torch.empty((4 * B, S, S, 4), dtype=torch.float32, device=dev)

    def kernel_percsim():
        C._lib.call("ps_consistency", v1, strides(v1), v2, strides(v2), 1, m1, m2, 1, maps, B, S, S, 1, pin, psnr, ws, nbytes)
    t_kernel_p = looped_ms(kernel_percsim, args.iters, 5) * 1e3
    t_torch = looped_ms(lambda: torch_formula(v1, v2, m1, m2, maps), max(5, args.iters // 5), 5) * 1e3
    kernel()
    diff = float((psnr - torch_formula(v1, v2, m1, m2, maps)).abs().max())
    print(json.dumps({"items": B, "size": S, "kernel_us": round(t_kernel, 1), "kernel_with_percsim_input_us": round(t_kernel_p, 1),
                      "torch_formula_us": round(t_torch, 1), "speedup": round(t_torch / t_kernel, 1),
                      "host_fit_us": round(t_fit, 1), "max_psnr_diff_db": diff}))


if __name__ == "__main__":
    main()
