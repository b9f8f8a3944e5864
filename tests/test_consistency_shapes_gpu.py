"""GPU: the homography consistency pass (csrc/consistency.hip) off 256 x 256 squares, against its float32 numpy twin
(tests/_consistency_twin.py), bit for bit: RAW mode's two images at every shape, map family, mask kind and view dtype of the twin's case
table (one pixel, one row of 18 tiles, partial tiles both ways, block edges inside tiles, a transposed pair); PSNR per direction from the
twin's fp64 sums; PERCSIM mode's standardisation; storage other than dense NCHW; the finish kernel's second workgroup; the clamp of
the mask sum; non-finite pixels; the cut into launches; and PercSim_vis at 256 x 512, the one non-square size PNet's HIP path takes.

The twin itself is held against the fp64 restatement on the CPU (tests/test_consistency_twin_cpu.py): its warp is within 3.82e-5 of
warp64 on the 0-255 scale over every shape here (bound BOUND_WARP = 1e-4; from the operations 3.8e-5), its PSNR within 2.5e-6 dB.

What is exact and what is not.  Every stage of k_consistency_tiles is compared with np.array_equal on the bit patterns (any two NaNs
count as equal): fp64 and fp32 multiply, add and divide are IEEE on both sides.  The one operation a host cannot reproduce is the fp64
log10 of k_consistency_finish (the device's math library against numpy's, neither correctly rounded), and the tile sums it takes are
added in another order than the twin's: PSNR is therefore allowed 1 ulp of its fp32 result, and must be equal wherever the twin's fp64
value is further than 1e-9 relative from an fp32 rounding boundary.
No stage of k_consistency_tiles needed the 1 ulp: on the MI355X every one of them is the twin's bits.
"""
import functools

import numpy as np
import pytest
import torch

import _consistency_twin as T
import percsim_ref64 as PR
from pixelsynth_amd import _images, consistency as C, synthetic as syn
from pixelsynth_amd.networks.pretrained_networks import PNet
from test_consistency_gpu import BOUND_PERCSIM, DEV, t

pytestmark = pytest.mark.gpu
IDS = ["%dx%d" % s for s in T.SHAPES]
# Bounds, and the maxima measured on the MI355X (printed by the tests): PSNR per direction against psnr_of of the twin's sums 0 ulp in
# every case of this file, bound 1 ulp (0 where the fp64 value is clear of a rounding boundary); PercSim_vis at 256 x 512 against PNet's
# torch formula on the twin's inputs 5.96e-8, bound BOUND_PERCSIM = 1e-6 (tests/test_consistency_gpu.py).
PSNR_ULP = 1


def launch(view1, view2, mask1, mask2, maps, mode=C.PERCSIM_RAW):
    """One launch on device tensors -> (psnr (B, 2), pin (2, B, 2, H, W, 4) fp32: the a and the b image of every item and direction)"""
    B, _, H, W = view1.shape
    pin = torch.full((4 * B, H, W, 4), -7.0, dtype=torch.float32, device=DEV)
    psnr = torch.full((B, 2), -7.0, dtype=torch.float32, device=DEV)
    C._launch(view1, view2, mask1, mask2, t(maps), mode, pin, psnr)
    torch.cuda.synchronize()
    return psnr.cpu().numpy(), pin.view(2, B, 2, H, W, 4).cpu().numpy()


def same_bits(got, want):
    """fp32 arrays equal bit for bit, any two NaNs counting as equal"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | both_nan).all())


def check_images(pin, ta, tb, what, transform=None):
    for name, got, want in (("a", pin[0], ta), ("b", pin[1], tb)):
        if transform is not None:
            want = np.stack([transform(want[..., j], j) for j in range(3)], -1)
        if not same_bits(got[..., :3], want):
            bad = np.argwhere(~((got[..., :3].view(np.uint32) == np.ascontiguousarray(want).view(np.uint32))
                                | (np.isnan(got[..., :3]) & np.isnan(want))))
            i = tuple(bad[0])
            raise AssertionError("%s: image %s differs at %d of %d values, first at (item, direction, y, x, channel) = %s: "
                                 "got %r, twin %r" % (what, name, len(bad), want.size, i, got[..., :3][i], want[i]))
        assert not got[..., 3].any(), (what, name, "lane 3 must be 0")


def check_psnr(psnr, sums, what):
    """-> the largest ulp distance.  Within PSNR_ULP of the twin's, and equal where the fp64 value is clear of a rounding boundary."""
    worst = 0
    for idx in np.ndindex(*psnr.shape):
        sd, sm = sums[idx]
        want, d = T.psnr_of(sd, sm), T.ulp_distance(psnr[idx], T.psnr_of(sd, sm))
        assert d <= PSNR_ULP, (what, idx, float(psnr[idx]), float(want))
        if T.rounding_is_safe(T.psnr64_of(sd, sm)):
            assert d == 0, (what, idx, float(psnr[idx]), float(want), "clear of a rounding boundary: must be equal")
        worst = max(worst, d)
    return worst


@functools.lru_cache(maxsize=None)
def twin_of(H, W, family, kind, dtype):
    v1, v2 = T.views(H, W, dtype)
    m1, m2 = T.masks(H, W, kind)
    maps = T.family_maps(H, W, family)
    return (v1, v2, m1, m2, maps) + T.twin_batch(v1, v2, m1, m2, maps)


@pytest.mark.parametrize("H,W", T.SHAPES, ids=IDS)
def test_raw_mode_and_psnr_bit_for_bit(H, W):
    worst = 0
    for family in T.FAMILIES:
        for kind in T.MASK_KINDS:
            for dtype in (np.uint8, np.float32):
                v1, v2, m1, m2, maps, ta, tb, sums = twin_of(H, W, family, kind, dtype)
                what = "%d x %d, %s maps, %s mask, %s views" % (H, W, family, kind, np.dtype(dtype).name)
                psnr, pin = launch(t(v1), t(v2), t(m1), t(m2), maps)
                check_images(pin, ta, tb, what)
                worst = max(worst, check_psnr(psnr, sums, what))
    print("%d x %d: PSNR at most %d ulp from the twin" % (H, W, worst))


@pytest.mark.parametrize("H,W", [(3, 7), (37, 130)], ids=["3x7", "37x130"])
def test_percsim_mode_is_the_standardised_raw_image(H, W):
    for family in ("mild", "outside"):
        for dtype in (np.uint8, np.float32):
            v1, v2, m1, m2, maps, ta, tb, sums = twin_of(H, W, family, "f32", dtype)
            psnr, pin = launch(t(v1), t(v2), t(m1), t(m2), maps, C.PERCSIM)
            check_images(pin, ta, tb, "PERCSIM mode, %d x %d, %s" % (H, W, family), T.standardised)
            check_psnr(psnr, sums, "PERCSIM mode")
            # the RGB constants on the BGR-ordered channels: taking them in RGB order would be another image
            assert not np.array_equal(T.standardised(ta[..., 0], 0), T.standardised(ta[..., 0], 2))


def _layouts(x):
    """A (B, 3, H, W) device tensor in other storage, the same values: channels-last, and a crop of a larger tensor (sB and sH off
    the dense values)"""
    B, _, H, W = x.shape
    big = torch.full((B, 3, H + 5, W + 9), 77, dtype=x.dtype, device=DEV)
    big[:, :, 2:2 + H, 3:3 + W] = x
    crop = big[:, :, 2:2 + H, 3:3 + W]
    assert crop.stride(0) != 3 * H * W and crop.stride(2) != W
    return {"channels-last": x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), "crop": crop}


@pytest.mark.parametrize("H,W", [(37, 130), (130, 37)], ids=["37x130", "130x37"])
def test_storage_other_than_dense_nchw(H, W):
    for dtype in (np.uint8, np.float32):
        v1, v2, m1, m2, maps, ta, tb, sums = twin_of(H, W, "mild", "u8_bytes", dtype)
        d1, d2, dm1, dm2 = t(v1), t(v2), t(m1), t(m2)
        psnr, pin = launch(d1, d2, dm1, dm2, maps)
        check_images(pin, ta, tb, "dense")
        L1, L2 = _layouts(d1), _layouts(d2)
        for name, (a, b) in {"channels-last": (L1["channels-last"], L2["channels-last"]), "crop": (L1["crop"], L2["crop"]),
                             "view 1 channels-last, view 2 a crop": (L1["channels-last"], L2["crop"]),
                             "view 1 a crop, view 2 dense": (L1["crop"], d2)}.items():
            assert torch.equal(a, d1) and torch.equal(b, d2)
            p, x = launch(a, b, dm1, dm2, maps)
            assert same_bits(p, psnr) and same_bits(x, pin), (name, np.dtype(dtype).name)
        # one image for the whole batch, expanded with stride 0, against the same image repeated densely
        e1 = d1[1:2].expand(T.B, 3, H, W)
        assert e1.stride(0) == 0
        p, x = launch(e1, d2, dm1, dm2, maps)
        q, y = launch(e1.contiguous(), d2, dm1, dm2, maps)
        assert same_bits(p, q) and same_bits(x, y)
        assert same_bits(p[1], psnr[1]) and same_bits(x[:, 1], pin[:, 1]) and not same_bits(x[:, 0], pin[:, 0])
        # and the front end hands the strides on
        H12, H21, back = T.forward_of(maps)
        rows = C.consistency_rows(d1, d2, dm1, dm2, H12, H21)
        assert torch.equal(C.consistency_rows(L1["crop"], L2["channels-last"], dm1, dm2, H12, H21), rows)
        check_psnr(rows[:, :2].cpu().numpy(), T.twin_batch(v1, v2, m1, m2, back)[2], "consistency_rows")


def test_finish_kernel_second_workgroup():
    # B = 33 at 6 x 70: 66 (item, direction) rows, so k_consistency_finish runs two workgroups, over 4 tiles each row
    H, W, n = 6, 70, 33
    v1, v2 = T.views(H, W, np.uint8, n)
    m1, m2 = T.masks(H, W, "f32", n)
    H12, H21, maps = T.forward_of(T.family_maps(H, W, "mild", n))
    d = [t(x) for x in (v1, v2, m1, m2)]
    rows = C.consistency_rows(*d, H12, H21)
    assert rows.shape == (n, 3)
    for i in range(n):
        alone = C.consistency_rows(*(x[i:i + 1] for x in d), H12[i:i + 1], H21[i:i + 1])
        assert torch.equal(alone[0], rows[i]), i
    got = rows.cpu().numpy()
    worst = check_psnr(got[:, :2], T.twin_batch(v1, v2, m1, m2, maps)[2], "B = 33")
    assert np.array_equal(got[:, 2], (0.5 * (got[:, 0].astype(np.float64) + got[:, 1])).astype(np.float32))
    assert len(np.unique(got[:, :2])) == 2 * n, "every row its own value: a row read from another item's sums would show"
    print("B = 33 at 6 x 70: PSNR at most %d ulp from the twin" % worst)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 7)], ids=["1x1", "3x7"])
def test_mask_sum_below_one_is_clamped(H, W):
    v1, v2 = T.views(H, W, np.float32)
    rs = np.random.RandomState(H * W)
    m1, m2 = ((rs.uniform(0.2, 0.7, (T.B, 1, H, W)) / (H * W)).astype(np.float32) for _ in range(2))
    maps = np.tile(np.eye(3).ravel(), (T.B, 2, 1))          # the identity: every pixel is compared with another view's pixel
    ta, tb, sums = T.twin_batch(v1, v2, m1, m2, maps)
    psnr, pin = launch(t(v1), t(v2), t(m1), t(m2), maps)
    check_images(pin, ta, tb, "mask sum in (0, 1)")
    check_psnr(psnr, sums, "mask sum in (0, 1)")
    for idx in np.ndindex(T.B, 2):
        sd, sm = sums[idx]
        assert 0.0 < sm < 1.0 and sd > 0.0
        assert T.psnr64_of(sd, sm) == 10.0 * np.log10(1.0 / (sd / (3.0 * 1.0)))            # the denominator is 3 * 1
        unclamped = 10.0 * np.log10(1.0 / (sd / (3.0 * sm)))
        assert abs(float(psnr[idx]) - unclamped) > 1.0, "the case must depend on the clamp (dB)"


def test_non_finite_pixels_stay_in_their_item():
    H, W = 12, 200
    v1, v2, m1, m2, maps, ta, tb, sums = twin_of(H, W, "mild", "f32", np.float32)
    clean_psnr, clean = launch(t(v1), t(v2), t(m1), t(m2), maps)
    check_images(clean, ta, tb, "clean")
    w1, w2 = v1.copy(), v2.copy()
    w1[1, 0, 5, 100], w1[1, 2, 7, 30] = np.nan, np.inf
    w2[1, 1, 3, 150] = -np.inf
    na, nb, nsums = T.twin_batch(w1, w2, m1, m2, maps)
    assert np.isnan(na[1]).any() and np.isnan(nb[1]).any() and np.isinf(na[1]).any() and np.isnan(nsums[1, :, 0]).all()
    assert np.isfinite(na[[0, 2]]).all() and np.isfinite(nb[[0, 2]]).all()
    psnr, pin = launch(t(w1), t(w2), t(m1), t(m2), maps)
    check_images(pin, na, nb, "a NaN and two Inf pixels in item 1")          # NaN where the twin has NaN, and nowhere else
    assert np.isnan(psnr[1]).all() and check_psnr(psnr, nsums, "non-finite") <= PSNR_ULP
    for i in (0, 2):
        assert same_bits(pin[:, i], clean[:, i]) and same_bits(psnr[i], clean_psnr[i]), i
    H12, H21, back = T.forward_of(maps)
    rows = C.consistency_rows(t(w1), t(w2), t(m1), t(m2), H12, H21).cpu().numpy()
    assert np.isnan(rows[1]).all() and np.isfinite(rows[[0, 2]]).all()
    check_psnr(rows[:, :2], T.twin_batch(w1, w2, m1, m2, back)[2], "non-finite, consistency_rows")


def test_launch_cuts_do_not_change_a_row(monkeypatch):
    H, W, n = 12, 200, 5
    v1, v2 = T.views(H, W, np.uint8, n)
    m1, m2 = T.masks(H, W, "u8_bytes", n)
    H12, H21, maps = T.forward_of(T.family_maps(H, W, "mild", n))
    d = [t(x) for x in (v1, v2, m1, m2)]
    whole = C.consistency_rows(*d, H12, H21)
    launches = []
    real = C._launch
    monkeypatch.setattr(C, "_launch", lambda *a: (launches.append(a[0].shape[0]), real(*a))[1])
    monkeypatch.setattr(_images, "MAX_B", 2)
    cut = C.consistency_rows(*d, H12, H21)
    assert launches == [2, 2, 1]
    assert torch.equal(cut, whole)
    check_psnr(whole[:, :2].cpu().numpy(), T.twin_batch(v1, v2, m1, m2, maps)[2], "B = 5")


@pytest.fixture(scope="module")
def pnet():
    torch.cuda.set_device(DEV)
    sd = {k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(PR.WEIGHT_SEED).items()}
    return PNet(use_gpu=True, weights=sd)


def test_percsim_vis_at_256_x_512(pnet):
    H, W = 256, 512
    probe = torch.empty((1, 3, H, W), dtype=torch.float32, device=DEV)
    assert pnet.hip_takes(probe, probe), "256 x 512 must run PercSim's HIP path (the kernel's own standardisation)"
    v1, v2 = T.views(H, W, np.uint8, 1)
    m1, m2 = T.masks(H, W, "f32", 1)
    H12, H21, maps = T.forward_of(T.family_maps(H, W, "mild", 1)[:, ::-1])      # (direction 0 the random map, not the tie map)
    rows = C.consistency_rows(t(v1), t(v2), t(m1), t(m2), H12, H21, pnet=pnet).cpu().numpy()
    ta, tb, sums = T.twin_batch(v1, v2, m1, m2, maps)
    check_psnr(rows[:, :2], sums, "256 x 512")
    with torch.no_grad():
        want = pnet.torch_forward(t(ta[0].transpose(0, 3, 1, 2)), t(tb[0].transpose(0, 3, 1, 2))).cpu().numpy()
    err = float(np.abs(rows[0, 3:5].astype(np.float64) - want.astype(np.float64)).max())
    print("percsim_vis at 256 x 512: max error against the torch formula on the twin's inputs: %.3g" % err)
    assert err <= BOUND_PERCSIM
    assert rows[0, 5] == np.float32(0.5 * (np.float64(rows[0, 3]) + np.float64(rows[0, 4])))
    assert rows[0, 3] != rows[0, 4] and (rows[0, 3:5] > 0.01).all()
