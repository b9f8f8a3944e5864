"""GPU: the homography consistency score on the HIP path (csrc/consistency.hip) against the fp64 restatement
(tests/golden/consistency_ref64.py, tests/golden/consistency.npz): the warp's values (exact for the identity and integer shifts, maps
reaching outside the source, a row where W crosses 0), PSNR_vis per direction with the clamp and the m^2 weighting, PercSim_vis against
PNet's torch formula on the restatement's BGR inputs, dtypes and bit-level reproducibility, and the CLI on one rank and two."""
import json
import os

import numpy as np
import pytest
import torch

import consistency_ref64 as R
import percsim_ref64 as PR
from pixelsynth_amd import consistency as C, synthetic as syn
from pixelsynth_amd.networks.pretrained_networks import PNet
from test_metrics_gpu import _cli

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# Bounds, and the maxima measured on the MI355X (printed by the tests): the warp against fp64 on the 0-255 scale (fp32 bilinear sum and
# the fp32 steps of the readback) 7.6e-6, bound 1e-4; PSNR_vis against fp64 1.7e-5 dB, bound 1e-3 dB (a difference of nearly equal
# images amplifies the fp32 warp's rounding); PercSim_vis against PNet's fp32 torch formula on the fp64 restatement's inputs 6.7e-8,
# bound 1e-6, while feeding the same data in RGB order moves the score by 7.8e-5.
BOUND_WARP, BOUND_PSNR, BOUND_PERCSIM = 1e-4, 1e-3, 1e-6


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def pnet():
    torch.cuda.set_device(DEV)
    sd = {k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(PR.WEIGHT_SEED).items()}
    net = PNet(use_gpu=True, weights=sd)
    probe = torch.empty((1, 3, 256, 256), dtype=torch.float32, device=DEV)
    assert net.hip_takes(probe, probe), "the tests below must run PercSim's HIP path (the kernel's own standardisation)"
    return net


def raw_pass(view1, view2, mask1, mask2, maps):
    """One launch in PS_CONSISTENCY_PERCSIM_RAW mode -> (psnr (B, 2), a, b (B, 2, H, W, 3) fp32: t * 2 - 1 of the compared images)"""
    B, _, H, W = view1.shape
    pin = torch.empty((4 * B, H, W, 4), dtype=torch.float32, device=DEV)
    psnr = torch.empty(B, 2, dtype=torch.float32, device=DEV)
    C._launch(view1, view2, mask1, mask2, t(maps), C.PERCSIM_RAW, pin, psnr)
    x = pin.view(2, B, 2, H, W, 4)[..., :3].cpu().numpy()
    assert (pin[..., 3] == 0).all()
    return psnr.cpu().numpy(), x[0], x[1]


def maps_of(Hs):
    """per-item map pairs (B, 2, 9) from (B, 2, 3, 3) forward homographies"""
    return np.stack([C.invert_map(Hs[:, k]) for k in (0, 1)], 1).reshape(len(Hs), 2, 9)


def test_identity_and_integer_shifts_are_exact():
    v = R.smooth_view(31, 2)
    ones = np.ones((2, 1, 256, 256), np.float32)
    ident = np.tile(np.eye(3), (2, 2, 1, 1))
    psnr, a, b = raw_pass(t(v), t(v), t(ones), t(ones), maps_of(ident))
    assert (psnr == 100.0).all() and np.array_equal(a, b)
    for dx, dy in ((3, 0), (-5, 7), (0, -2)):
        T = np.array([[1.0, 0, dx], [0, 1.0, dy], [0, 0, 1.0]])
        _, a, _ = raw_pass(t(v), t(v), t(ones), t(ones), maps_of(np.tile(T, (2, 2, 1, 1))))
        for b_ in range(2):
            tr = R.try_bgr(v[b_])                                      # view 1 (direction 1's source) warped by T: shifted by (dx, dy)
            want = np.zeros_like(tr)
            ys, xs = slice(max(dy, 0), 256 + min(dy, 0)), slice(max(dx, 0), 256 + min(dx, 0))
            yr, xr = slice(max(-dy, 0), 256 + min(-dy, 0)), slice(max(-dx, 0), 256 + min(-dx, 0))
            want[ys, xs] = tr[yr, xr]
            ta = ((want / np.float32(255)).astype(np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
            assert np.array_equal(a[b_, 1], ta), (dx, dy)


def test_warp_values_against_fp64():
    v1, v2 = R.smooth_view(41, 3), R.smooth_view(42, 3)
    ones = np.ones((3, 1, 256, 256), np.float32)
    Hs = np.stack([np.stack([R.rotation_homography((4.0, -3.0, 2.0)), R.rotation_homography((-6.0, 2.0, 0.0))]),
                   np.stack([np.array([[1.3, 0.1, -60.0], [-0.05, 1.2, 40.0], [0, 0, 1.0]]),     # part of the frame from outside
                             np.array([[0.8, 0, 200.0], [0, 0.8, -90.0], [0, 0, 1.0]])]),
                   np.stack([np.linalg.inv(np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0 / 128, 0, -1.0]])),  # W crosses 0 at x = 128
                             np.linalg.inv(np.array([[1.0, 0.2, 3.0], [0.0, 1.0, 0], [0, -1.0 / 100, 1.0]]))])])
    maps = maps_of(Hs)
    _, a, _ = raw_pass(t(v1), t(v2), t(ones), t(ones), maps)
    worst = 0.0
    for b in range(3):
        for k, src in ((0, v2[b]), (1, v1[b])):
            want = R.warp64(R.try_bgr(src), maps[b, k])
            got = (a[b, k].astype(np.float64) + 1.0) / 2.0 * 255.0
            worst = max(worst, float(np.abs(got - want).max()))
    print("warp max error against fp64 (0-255 scale):", "%.3g" % worst)
    assert worst <= BOUND_WARP
    sx, _, _, _ = R.source_positions(maps[2, 0], 256, 256)
    assert (sx[:, 128] == 0).all() and (sx[:, 127] < -1000).all()       # W = 0 exactly, and saturated next to it


def _golden_rows(case, dtype=torch.uint8, pnet=None):
    z = R.case_inputs(case)
    if dtype == torch.float32:     # x / 255 on the host, as TF.to_tensor (the device may multiply by 1 / 255 instead)
        v1, v2 = (t(torch.from_numpy(z[k]).float().div(255).numpy()) for k in ("view1", "view2"))
    else:
        v1, v2 = t(z["view1"]), t(z["view2"])
    rows = C.consistency_rows(v1, v2, t(z["mask1"]), t(z["mask2"]), points=(list(z["reproj1"]), list(z["reproj2"])), pnet=pnet)
    return z, rows


def test_psnr_vis_against_fp64(golden_dir):
    g = np.load(os.path.join(golden_dir, "consistency.npz"))
    worst = 0.0
    for case in R.CASES:
        z, rows = _golden_rows(case)
        got = rows.cpu().double().numpy()
        want = g["psnr64/" + case[0]]
        worst = max(worst, float(np.abs(got[:, :2] - want).max()))
        assert np.abs(got[:, :2] - want).max() <= BOUND_PSNR, (case[0], got[:, :2], want)
        assert np.array_equal(got[:, 2], (0.5 * (got[:, 0] + got[:, 1])).astype(np.float32).astype(np.float64))
        if case[5] == "empty":
            assert (got[:, :3] == 100.0).all()
        if case[5] == "fractional":        # the mask weights the difference twice: m^2 differs from m by far more than the bound
            H12, H21, _ = R.case64(case, z)
            d0 = R.direction64(z["view2"][0], z["view1"][0], z["mask1"][0], C.invert_map(H21)[0].ravel())
            m = R.mask_unit(z["mask1"][0]).astype(np.float64)
            once = 10 * np.log10(3.0 * max(m.sum(), 1.0) / ((d0[2] - d0[3]) ** 2).sum())
            assert abs(once - got[0, 0]) > 100 * BOUND_PSNR
    print("psnr_vis max error against fp64 (dB):", "%.3g" % worst)


def test_percsim_vis_against_torch_formula(pnet):
    case = R.CASES[1]
    z, rows = _golden_rows(case, pnet=pnet)
    rows = rows.cpu().double().numpy()
    H12, H21, _ = R.case64(case, z)
    worst, worst_rgb = 0.0, float("inf")
    for b in range(case[2]):
        _, ab = R.item64(z["view1"][b], z["view2"][b], z["mask1"][b], z["mask2"][b], H12[b], H21[b])
        x0 = t(np.stack([a for a, _ in ab]).astype(np.float32))
        x1 = t(np.stack([b_ for _, b_ in ab]).astype(np.float32))
        with torch.no_grad():
            want = pnet.torch_forward(x0 * 2 - 1, x1 * 2 - 1).cpu().double().numpy()
            rgb = pnet.torch_forward(x0.flip(1) * 2 - 1, x1.flip(1) * 2 - 1).cpu().double().numpy()
        worst = max(worst, float(np.abs(rows[b, 3:5] - want).max()))
        worst_rgb = min(worst_rgb, float(np.abs(rows[b, 3:5] - rgb).max()))
        assert rows[b, 5] == np.float32(0.5 * (rows[b, 3] + rows[b, 4]))
    print("percsim_vis max error against the torch formula:", "%.3g" % worst, " RGB-ordered input differs by", "%.3g" % worst_rgb)
    assert worst <= BOUND_PERCSIM
    assert worst_rgb > 10 * BOUND_PERCSIM, "the BGR quirk must change the score"


def test_percsim_vis_torch_path_agrees(pnet):
    # with the split-fp16 convolutions forced off (what the overflow guard's rerun does), the kernel writes the [-1, 1] inputs and
    # PNet's torch formula scores them: the PSNR columns are the same bits, PercSim agrees within the bound
    from pixelsynth_amd.networks import f16x3
    case = R.CASES[1]
    _, hip = _golden_rows(case, pnet=pnet)
    with f16x3.decoder_conv("fp32"):
        probe = torch.empty((1, 3, 256, 256), dtype=torch.float32, device=DEV)
        assert not pnet.hip_takes(probe, probe)
        _, tor = _golden_rows(case, pnet=pnet)
    assert torch.equal(tor[:, :3], hip[:, :3])
    assert float((tor[:, 3:] - hip[:, 3:]).abs().max()) <= BOUND_PERCSIM


def test_dtypes_and_bit_reproducibility(pnet):
    case = R.CASES[0]
    z, u8 = _golden_rows(case, pnet=pnet)
    _, f32 = _golden_rows(case, torch.float32, pnet=pnet)
    assert torch.equal(u8, f32), "uint8 and fp32 views"
    v1, v2, m1, m2 = (t(z[k]) for k in ("view1", "view2", "mask1", "mask2"))
    H12, H21 = C.fit_points(list(z["reproj1"]), list(z["reproj2"]))
    fm1, fm2 = (t(torch.from_numpy(z[k]).float().div(255).numpy()) for k in ("mask1", "mask2"))
    assert torch.equal(C.consistency_rows(v1, v2, fm1, fm2, H12, H21, pnet=pnet), u8), "uint8 and fp32 masks"
    assert torch.equal(C.consistency_rows(v1, v2, m1, m2, H12, H21, pnet=pnet), u8), "run to run"
    # batch position and size: item 1 alone, and items in another order inside a larger batch
    one = C.consistency_rows(v1[1:], v2[1:], m1[1:], m2[1:], H12[1:], H21[1:], pnet=pnet)
    assert torch.equal(one[0], u8[1])
    idx = [1, 0, 1]
    big = C.consistency_rows(v1[idx], v2[idx], m1[idx], m2[idx], H12[idx], H21[idx])
    assert torch.equal(big[:, :3], u8[idx, :3])
    # channels-last storage read in place
    cl = C.consistency_rows(v1.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), v2, m1, m2, H12, H21)
    assert torch.equal(cl, u8[:, :3])


def _write_tree(root, cases):
    from PIL import Image
    dirs, n = [], 0
    rs = np.random.RandomState(5)
    for case in cases:
        z = R.case_inputs(case)
        for b in range(case[2]):
            d = int(rs.randint(0, 8))
            dirs.append(d)
            for sub in ("views", "masks"):
                os.makedirs(os.path.join(root, sub, "%04d" % n))
            for k, v in ((1, z["view1"][b]), (2, z["view2"][b])):
                Image.fromarray(np.ascontiguousarray(v.transpose(1, 2, 0))).save(
                    os.path.join(root, "views", "%04d" % n, "output_image_%s_000%d.png" % (C.MAPPING[d], k)))
            for k, m in ((1, z["mask1"][b]), (2, z["mask2"][b])):
                Image.fromarray(np.repeat(m[0][..., None], 3, 2)).save(os.path.join(root, "masks", "%04d" % n, "mask%d.png" % k))
            os.makedirs(os.path.join(root, "points"), exist_ok=True)
            np.save(os.path.join(root, "points", "reproj1_%d.npy" % n), z["reproj1"][b])
            np.save(os.path.join(root, "points", "reproj2_%d.npy" % n), z["reproj2"][b])
            n += 1
    np.save(os.path.join(root, "dirs.npy"), np.array(dirs))
    return n


def test_cli_end_to_end(tmp_path, golden_dir, pnet):
    from pixelsynth_amd.evaluate import consistency_summarize
    root = str(tmp_path)
    cases = [c for c in R.CASES if c[5] == "valid"]
    n = _write_tree(root, cases)
    g = np.load(os.path.join(golden_dir, "consistency.npz"))
    want64 = np.concatenate([g["psnr64/" + c[0]] for c in cases])
    wpath = str(tmp_path / "vgg16.pth")
    torch.save({k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(PR.WEIGHT_SEED).items()}, wpath)
    base = ["--consistency", os.path.join(root, "views"), "--masks", os.path.join(root, "masks"), "--points",
            os.path.join(root, "points"), "--directions", os.path.join(root, "dirs.npy"), "--batch", "3"]
    one, two = str(tmp_path / "one.json"), str(tmp_path / "two.json")
    out1 = _cli(base + ["--json", one, "--vgg16", wpath])
    out2 = _cli(base + ["--json", two, "--vgg16", wpath], env={"PS_DRYRUN_ONE_GPU": "1"}, nproc=2)
    d1, d2 = json.load(open(one)), json.load(open(two))
    assert d1["n"] == n and d1["rows"] == d2["rows"] and d1["means"] == d2["means"]
    rows = np.array([[r[c] for c in C.COLUMNS] for r in d1["rows"]])
    means = consistency_summarize(rows, True)
    lines = [ln for ln in out1.splitlines() if " \t " in ln]
    assert lines == ["%s \t %0.5f" % kv for kv in means.items()] and lines[0].startswith("PercSim_vis"), out1
    assert [ln for ln in out2.splitlines() if " \t " in ln] == lines
    assert np.abs(rows[:, :2] - want64).max() <= BOUND_PSNR
    assert abs(means["PSNR_vis"] - float(np.mean(0.5 * want64.sum(1)))) <= BOUND_PSNR
    plain = _cli(base)
    assert [ln for ln in plain.splitlines() if " \t " in ln] == ["PSNR_vis \t %0.5f" % means["PSNR_vis"]]
