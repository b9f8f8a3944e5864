"""CPU: the homography consistency score's host side -- find_homography (cv2.findHomography with method 0, restated), the reference's
point conversion and two separate fits, the golden file against the fp64 restatement, the C ABI of the consistency library, and the
CLI's discovery and argument checks, before any device is touched."""
import json
import os

import numpy as np
import pytest

from abi_util import assert_library_matches_header
import consistency_ref64 as R
from pixelsynth_amd import _lib, consistency as C, evaluate



def _known(seed=0, n=30, deg=(3.0, -2.0, 1.0)):
    Ht = R.rotation_homography(deg)
    Ht = Ht / Ht[2, 2]
    src = np.random.RandomState(seed).uniform(0, 255, (n, 2))
    return Ht, src, R.apply_h(Ht, src)


def forward_error(H, src, dst):
    return float(((R.apply_h(H, src) - dst) ** 2).sum())


def test_find_homography_recovers_a_known_h():
    for n in (4, 5, 30):
        Ht, src, dst = _known(n=n)
        H = C.find_homography(src, dst)
        assert np.abs(H - Ht).max() <= 1e-9 * np.abs(Ht).max(), n
    Hb = C.find_homography(np.stack([_known(1)[1], _known(2)[1]]), np.stack([_known(1)[2], _known(2)[2]]))
    assert Hb.shape == (2, 3, 3) and np.abs(Hb - _known()[0]).max() <= 1e-9 * np.abs(_known()[0]).max()


def test_find_homography_does_not_depend_on_point_order():
    Ht, src, dst = _known(3)
    noisy = dst + np.random.RandomState(4).randn(*dst.shape)
    H = C.find_homography(src, noisy)
    perm = np.random.RandomState(5).permutation(len(src))
    assert np.abs(C.find_homography(src[perm], noisy[perm]) - H).max() <= 1e-9 * np.abs(H).max()


def test_lm_solves_a_singular_system_by_pseudo_inverse():
    # solve(..., DECOMP_EIG): a singular damped system gives the minimum-norm step instead of an error
    A = np.diag([4.0, 1.0, 0.0])[None]
    P = C._pinv_eig(A)
    assert np.allclose(P[0], np.diag([0.25, 1.0, 0.0]), rtol=0, atol=1e-15)
    Ht, src, dst = _known(8, n=5)
    noisy = dst + 0.3 * np.random.RandomState(9).randn(*dst.shape)
    H = C._refine(C._dlt(src[None], noisy[None], [0]), src[None], noisy[None])
    assert np.isfinite(H).all() and forward_error(H[0], src, noisy) <= forward_error(C._dlt(src[None], noisy[None], [0])[0], src, noisy)


def test_lm_never_raises_the_forward_error():
    for seed in range(6):
        Ht, src, dst = _known(seed, n=12 + seed)
        noisy = dst + (0.5 + seed) * np.random.RandomState(10 + seed).randn(*dst.shape)
        dlt = C._dlt(src[None], noisy[None], [0])[0]
        H = C.find_homography(src, noisy)
        assert forward_error(H, src, noisy) <= forward_error(dlt, src, noisy), seed


def test_too_few_or_degenerate_points_raise_naming_the_item():
    Ht, src, dst = _known()
    with pytest.raises(ValueError, match="item 7: 3 point"):
        C.find_homography(src[:3], dst[:3], items=[7])
    line = np.c_[np.linspace(0, 200, 10), np.linspace(10, 110, 10)]
    with pytest.raises(ValueError, match="item 0: .*collinear"):
        C.find_homography(line, R.apply_h(Ht, line))
    same = np.tile([[5.0, 6.0]], (6, 1))
    with pytest.raises(ValueError, match="item 3: .*degenerate"):
        C.fit_points([R.to_raw(src[:6])] * 4, [R.to_raw(same)] * 4, items=[3, 4, 5, 6])


def test_points_to_pixels_and_two_separate_fits():
    raw = np.array([[-1.0, -1.0, 0.3], [1.0, 1.0, 0.2], [0.0, 0.5, 0.1]])
    p = C.points_to_pixels(raw)
    assert p.dtype == np.float32 and p.shape == (3, 2)
    # (p * 0.5 + 0.5) * 255 for both axes, then x -> 255 - x
    assert p.tolist() == [[255.0, 0.0], [0.0, 255.0], [127.5, 191.25]]
    r32 = raw.astype(np.float32)                     # a float32 array stays float32 through the arithmetic, as numpy keeps it
    assert C.points_to_pixels(r32).tolist() == p.tolist()
    Ht, src, dst = _known(6, n=20)
    noisy = dst + np.random.RandomState(7).randn(*dst.shape)
    H12, H21 = C.fit_points([R.to_raw(src)], [R.to_raw(noisy)])
    s32, d32 = src.astype(np.float32), noisy.astype(np.float32)
    assert np.allclose(H12[0], C.find_homography(s32, d32), rtol=0, atol=1e-6)
    assert np.allclose(H21[0], C.find_homography(d32, s32), rtol=0, atol=1e-6)
    inv = np.linalg.inv(H12[0])
    assert np.abs(H21[0] - inv / inv[2, 2]).max() > 1e-6, "h2 is its own fit, not inv(h)"


def test_invert_map_is_the_adjugate_inverse():
    Ht = _known()[0]
    Mi = C.invert_map(Ht[None])[0]
    assert np.abs(Mi @ Ht - np.eye(3)).max() < 1e-12
    with pytest.raises(ValueError, match="singular"):
        C.invert_map(np.zeros((1, 3, 3)))


def test_source_positions_of_simple_maps():
    sx, sy, fx, fy = R.source_positions(np.eye(3).ravel(), 8, 80)
    assert (sx == np.arange(80)).all() and (sy == np.arange(8)[:, None]).all() and not fx.any() and not fy.any()
    T = np.array([1, 0, 2.5, 0, 1, -1.25, 0, 0, 1.0])
    sx, sy, fx, fy = R.source_positions(T, 4, 8)
    assert (sx == np.arange(8) + 2).all() and (fx == 16).all() and (sy == np.arange(4)[:, None] - 2).all() and (fy == 24).all()
    # W crosses 0 along a row: W = 0 exactly reads the source's (0, 0), |W| tiny saturates far outside
    P = np.array([1, 0, 0, 0, 1, 0, 1.0, 0, -3.0])
    sx, sy, fx, fy = R.source_positions(P, 1, 8)
    assert sx[0, 3] == 0 and sy[0, 3] == 0 and fx[0, 3] == 0
    assert sx[0, 2] < 0 and sx[0, 4] > 0


def test_golden_file_matches_the_restatement(golden_dir):
    z = np.load(os.path.join(golden_dir, "consistency.npz"))
    assert json.loads(str(z["cases"])) == json.loads(json.dumps(R.CASES))
    for case in R.CASES:
        inp = R.case_inputs(case)
        assert float(sum(np.asarray(inp[k], np.float64).sum() for k in ("view1", "view2", "mask1", "mask2", "reproj1", "reproj2"))) \
            == float(z["sum/" + case[0]])
        H12, H21, psnr = R.case64(case, inp)
        for key, got in (("H12", H12), ("H21", H21)):
            want = z[key + "/" + case[0]]
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (case[0], key)
        assert np.allclose(psnr, z["psnr64/" + case[0]], rtol=1e-9, atol=0), case[0]
    assert (z["psnr64/empty_mask"] == 100.0).all()


def test_consistency_library_exports_its_header():
    assert_library_matches_header("consistency")
    L = _lib.library("consistency")
    assert _lib.call("ps_consistency_workspace_bytes", 3, 256, 256) == 3 * 2 * 256 * 2 * 8
    assert _lib.call("ps_consistency_workspace_bytes", 1, 5, 70) == 2 * 4 * 2 * 8          # tiles of 64 x 4: 2 x 2
    assert _lib.call("ps_consistency_workspace_bytes", 0, 256, 256) == 0
    with pytest.raises(RuntimeError, match="ps_consistency failed.*null"):
        _lib.call("ps_consistency", *([None] * 4 + [0, None, None, 0, None, 1, 256, 256, 0, None, None, None, 0]), stream=0)
    assert L.ps_consistency_last_error()


def test_consistency_library_refuses_sizes_and_alignment_before_any_launch():
    import ctypes
    strides = (ctypes.c_int64 * 4)(3 * 64, 64, 8, 1)
    p = 4096                                        # stands for a device pointer: every refusal below comes before one is read

    def call(H, W, mode=0, pin=None, ws_bytes=1 << 30):
        _lib.call("ps_consistency", p, strides, p, strides, 0, p, p, 0, p, 1, H, W, mode, pin, p, p, ws_bytes, stream=0)
    for H, W in ((32768, 8), (8, 32768), (0, 8), (8, 0), (40000, 40000)):     # sat_short's range: a column 32767 must stay outside
        with pytest.raises(RuntimeError, match=r"1 <= H, W <= 32767 required \(H = %d, W = %d\)" % (H, W)):
            call(H, W)
    with pytest.raises(RuntimeError, match="percsim_in must be 16-byte aligned"):
        call(8, 8, mode=1, pin=p + 8)
    with pytest.raises(RuntimeError, match="percsim_in must be 16-byte aligned"):
        call(8, 8, mode=2, pin=p + 4)
    with pytest.raises(RuntimeError, match="percsim_in goes with"):
        call(8, 8, mode=0, pin=p)
    with pytest.raises(RuntimeError, match="percsim_in goes with"):
        call(8, 8, mode=1, pin=None)
    with pytest.raises(RuntimeError, match="percsim_mode 3"):
        call(8, 8, mode=3, pin=p)
    # the largest sizes are taken as far as the workspace check (an aligned percsim_in with them)
    need = _lib.call("ps_consistency_workspace_bytes", 1, 32767, 32767)
    assert need == 2 * 512 * 8192 * 2 * 8
    with pytest.raises(RuntimeError, match="workspace of %d bytes required" % need):
        call(32767, 32767, mode=2, pin=p, ws_bytes=need - 1)


def test_consistency_rows_argument_checks():
    import torch
    a, m = torch.zeros(2, 3, 16, 16, dtype=torch.uint8), torch.zeros(2, 1, 16, 16, dtype=torch.uint8)
    H = np.tile(np.eye(3), (2, 1, 1))
    with pytest.raises(ValueError, match="differ in shape"):
        C.consistency_rows(a, a[:1], m, m, H, H)
    with pytest.raises(ValueError, match="mask2 must be"):
        C.consistency_rows(a, a, m, m[:, :, :8], H, H)
    with pytest.raises(TypeError, match="float32 or uint8"):
        C.consistency_rows(a, a, m.double(), m.double(), H, H)
    with pytest.raises(TypeError, match="float32 or both uint8"):
        C.consistency_rows(a.double(), a.double(), m, m, H, H)
    with pytest.raises(TypeError, match="PNet"):
        C.consistency_rows(a, a, m, m, H, H, pnet=object())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.consistency_rows(a, a, m, m, H, H)


def _tree(tmp_path, n=3, dirs=(0, 5, 7)):
    from PIL import Image
    v, m, p = (tmp_path / k for k in ("views", "masks", "points"))
    for i in range(n):
        (v / ("%04d" % i)).mkdir(parents=True)
        (m / ("%04d" % i)).mkdir(parents=True)
        for k in (1, 2):
            name = "output_image_%s_000%d.png" % (C.MAPPING[dirs[i]], k)
            Image.fromarray(np.full((256, 256, 3), 10 * k, np.uint8)).save(v / ("%04d" % i) / name)
            Image.fromarray(np.full((256, 256), 255, np.uint8)).save(m / ("%04d" % i) / ("mask%d.png" % k))
        p.mkdir(exist_ok=True)
        np.save(p / ("reproj1_%d.npy" % i), np.zeros((5, 3)))
        np.save(p / ("reproj2_%d.npy" % i), np.zeros((5, 3)))
    np.save(tmp_path / "dirs.npy", np.array(dirs[:n]))
    return str(v), str(m), str(p), str(tmp_path / "dirs.npy")


def test_cli_discovery_and_missing_files(tmp_path):
    v, m, p, d = _tree(tmp_path)
    items = evaluate.consistency_discover(v, m, p, d)
    assert [it[0] for it in items] == [0, 1, 2]
    assert items[1][1].endswith(os.path.join("0001", "output_image_UR_0001.png"))
    assert items[2][2].endswith(os.path.join("0002", "output_image_DL_0002.png"))
    assert items[0][3].endswith(os.path.join("0000", "mask1.png")) and items[0][6].endswith("reproj2_0.npy")
    assert len(evaluate.consistency_discover(v, m, p, d, max_img=2)) == 2
    with pytest.raises(ValueError, match="holds 3 directions"):
        evaluate.consistency_discover(v, m, p, d, max_img=4)
    os.remove(os.path.join(m, "0001", "mask2.png"))
    os.remove(os.path.join(p, "reproj1_2.npy"))
    with pytest.raises(FileNotFoundError, match=r"item 1: .*0001.mask2\.png is missing"):
        evaluate.consistency_discover(v, m, p, d)
    np.save(d, np.array([0, 8, 1]))
    with pytest.raises(ValueError, match="item 1: direction 8"):
        evaluate.consistency_discover(v, m, p, d, max_img=2)


def test_cli_decode_requires_256_frames(tmp_path):
    from PIL import Image
    v, m, p, d = _tree(tmp_path, n=1)
    item = evaluate.consistency_discover(v, m, p, d)[0]
    dec = evaluate._decode_item(item)
    assert dec[0].shape == (256, 256, 3) and dec[2].shape == (256, 256) and dec[2].dtype == np.uint8 and dec[4].shape == (5, 3)
    Image.fromarray(np.zeros((128, 256), np.uint8)).save(item[4])
    with pytest.raises(ValueError, match="mask2.png is 256 x 128.*256 x 256"):
        evaluate._decode_item(item)


def test_cli_decode_names_a_malformed_point_file(tmp_path):
    v, m, p, d = _tree(tmp_path, n=1)
    item = evaluate.consistency_discover(v, m, p, d)[0]
    for bad in (np.zeros(6), np.zeros((5, 1)), np.array([["a", "b"]] * 5)):
        np.save(item[6], bad)
        with pytest.raises(ValueError, match=r"item 0: .*reproj2_0\.npy holds .* \(n, >= 2\) real numbers"):
            evaluate._decode_item(item)


def test_check_keeps_free_labels_on_the_main_library():
    # callers label their checks freely ("pack", "conv", ...): a failure raises RuntimeError with libpixelsynth_hip.so's message
    with pytest.raises(RuntimeError, match=r"^some label failed \(rc=-1\): "):
        _lib.check(-1, "some label")
    _lib.check(0, "some label")
    with pytest.raises(RuntimeError, match=r"^ps_consistency failed \(rc=-2\): "):
        _lib.check(-2, "ps_consistency")
    with pytest.raises(KeyError):
        _lib.call("ps_no_such_entry_point")


def test_cli_argument_errors(tmp_path, capsys):
    cases = [(["--consistency", str(tmp_path)], "--consistency requires --masks, --points, --directions"),
             (["--consistency", str(tmp_path), "--masks", "m", "--points", "p", "--directions", "d", "--pred", "x"], "do not go with"),
             (["--pred", str(tmp_path), "--gt", str(tmp_path), "--masks", "m"], "--masks go with --consistency"),
             (["--pred", str(tmp_path)], "required: --gt")]
    for argv, msg in cases:
        with pytest.raises(SystemExit) as e:
            evaluate.main(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv


def test_cli_summary_is_the_reference_mean():
    rows = np.array([[30.0, 40.0, 35.0, 0.5, 0.25, 0.375], [100.0, 20.5, 60.25, 0.125, 0.0, 0.0625]])
    assert list(evaluate.consistency_summarize(rows)) == ["PSNR_vis"]
    s = evaluate.consistency_summarize(rows, percsim=True)
    assert list(s) == ["PercSim_vis", "PSNR_vis"]                 # METRICS order
    assert s["PSNR_vis"] == np.mean([35.0, 60.25]) and s["PercSim_vis"] == np.mean([0.375, 0.0625])


def test_evaluation_reexports_consistency_rows():
    from pixelsynth_amd import evaluation
    assert evaluation.consistency_rows is C.consistency_rows and evaluation.CONSISTENCY_COLUMNS == C.COLUMNS
    assert "homography consistency" not in evaluation.__doc__.split("are not provided")[0].split("FID")[-1]
