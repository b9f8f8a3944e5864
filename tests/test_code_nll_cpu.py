"""CPU-only: the host side of the likelihood of given codes (pixelsynth_amd/likelihood.py, csrc/code_nll.hip): the fp64 numpy definition
the GPU tests pin the kernel to (tests/golden/nll_ref64.py) against torch's cross entropy and closed forms, the C ABI of
libpixelsynth_nll.so against its header and bindings, the arithmetic of the result type, and the driver's --validate arguments."""
import json
import math

import numpy as np
import pytest
import torch

from abi_util import assert_library_matches_header
from nll_ref64 import code_nll_ref64, rounding_bound
from pixelsynth_amd import _lib, _libraries, driver, likelihood

LN2 = math.log(2.0)


@pytest.mark.parametrize("T", [1.0, 0.7])
def test_ref64_is_torch_cross_entropy_in_fp64(T):
    rs = np.random.RandomState(3)
    F_, L = 2, 37
    x = (3.0 * rs.randn(F_, 512, L)).astype(np.float32)
    t = rs.randint(0, 512, (F_, L))
    region = rs.randint(0, 2, (F_, L)).astype(np.uint8)
    ref = code_nll_ref64(x, t, region, T, "chw")
    xt = torch.from_numpy(x).double() / T
    want = torch.nn.functional.cross_entropy(xt, torch.from_numpy(t), reduction="none").numpy()
    np.testing.assert_allclose(ref["nll"], want, rtol=1e-13, atol=1e-13)
    logp = torch.log_softmax(xt, 1)
    np.testing.assert_allclose(ref["entropy"], -(logp.exp() * logp).sum(1).numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(ref["hit"], (xt.argmax(1).numpy() == t).astype(np.uint8))
    # the mean over all locations is nn.CrossEntropyLoss()
    assert abs(ref["frames"][:, :, 1].sum() / (F_ * L) - float(torch.nn.CrossEntropyLoss()(xt, torch.from_numpy(t)))) < 1e-13
    # the two layouts are one definition
    lc = code_nll_ref64(np.ascontiguousarray(x.transpose(0, 2, 1)), t, region, T, "lc")
    for k in ref:
        assert np.array_equal(ref[k], lc[k]), k
    # the frame table: the groups' own sums
    for f in range(F_):
        for g in (0, 1):
            sel = region[f] == g
            np.testing.assert_allclose(ref["frames"][f, g], [sel.sum(), ref["nll"][f][sel].sum(), ref["entropy"][f][sel].sum(),
                                                            ref["hit"][f][sel].sum()], rtol=1e-15)
    with pytest.raises(ValueError, match="layout 'hwc'"):
        code_nll_ref64(x, t, None, T, "hwc")


def test_ref64_closed_forms_and_invalid_values():
    L = 8
    x = np.zeros((1, 512, L), np.float32)
    x[0, :, 0] = 1.25                               # all equal: nll = entropy = ln 512, the arg-max is class 0
    x[0, 7, 1] = 80.0                               # one class ahead by 80, target on it ...
    x[0, 7, 2] = 80.0                               # ... and off it: nll = the gap
    x[0, :, 3] = -1e4
    x[0, 100, 3] = 1e4                              # magnitudes of 1e4: every other class underflows
    x[0, 5, 4] = x[0, 9, 4] = 2.0                   # a two-way tie: the lower class is the arg-max
    x[0, 3, 5] = np.nan
    t = np.array([[0, 7, 8, 100, 9, 4, -1, 512]])
    region = np.array([[0, 0, 1, 1, 1, 1, 0, 1]], np.uint8)
    ref = code_nll_ref64(x, t, region)
    ln512 = math.log(512.0)
    assert abs(ref["nll"][0, 0] - ln512) < 1e-14 and abs(ref["entropy"][0, 0] - ln512) < 1e-14 and ref["hit"][0, 0] == 1
    tail = math.log1p(511 * math.exp(-80.0))
    assert abs(ref["nll"][0, 1] - tail) < 1e-30 and ref["hit"][0, 1] == 1
    assert abs(ref["nll"][0, 2] - 80.0) < 1e-13 and ref["hit"][0, 2] == 0
    assert ref["nll"][0, 3] == 0.0 and ref["entropy"][0, 3] == 0.0 and ref["hit"][0, 3] == 1
    assert ref["hit"][0, 4] == 0 and code_nll_ref64(x, np.where(t == 9, 5, t))["hit"][0, 4] == 1
    assert abs(ref["nll"][0, 4] - (math.log(2 + 510 * math.exp(-2.0)))) < 1e-14
    assert np.isnan(ref["nll"][0, 5]) and np.isnan(ref["entropy"][0, 5])
    assert np.isnan(ref["nll"][0, 6]) and np.isnan(ref["nll"][0, 7]) and ref["hit"][0, 6] == ref["hit"][0, 7] == 0
    assert abs(ref["entropy"][0, 6] - ln512) < 1e-14            # (the distribution itself is fine where only the target is not)
    assert np.isnan(ref["frames"][0, 0, 1]) and np.isnan(ref["frames"][0, 1, 1])
    assert ref["frames"][0, 0, 0] == 3 and ref["frames"][0, 1, 0] == 5 and ref["frames"][0, 0, 3] == 2 and ref["frames"][0, 1, 3] == 1
    # temperature: the gap scales
    assert abs(code_nll_ref64(x, t, None, 0.5)["nll"][0, 2] - 160.0) < 1e-13
    # an empty group: zeros, never NaN
    none = code_nll_ref64(x[:, :, :5], t[:, :5])
    assert np.array_equal(none["frames"][0, 1], np.zeros(4)) and none["frames"][0, 0, 0] == 5
    # the bound: 2^-23 (2 max|x / T| + 32)
    b = rounding_bound(x, 0.5)
    assert b.shape == (1, L) and b[0, 3] == 2.0 ** -23 * (2 * 2e4 + 32) and b[0, 5] == 2.0 ** -23 * 32


def test_the_registry_has_the_nll_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "nll")
    assert entry.so == "libpixelsynth_nll.so" and entry.headers == ("pixelsynth_nll.h",) and entry.last_error == "ps_nll_last_error"
    assert [u for u, _ in entry.units] == ["code_nll.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("nll")
    assert set(protos) == set(_lib.NLL_PROTOS) == {"ps_nll_last_error", "ps_code_nll_f32"}
    assert likelihood.CLASSES == 512 and likelihood.LAYOUTS == ("chw", "lc")


def test_code_nll_refuses_before_anything_is_launched():
    L = _lib.library("nll")
    err = L.ps_nll_last_error
    x = torch.zeros(8)
    p = x.data_ptr()                                   # (any non-null address: the arguments are refused before it is looked at)
    call = lambda *a: L.ps_code_nll_f32(*a, None)
    assert call(None, 0, p, None, 1.0, 1, 4, p, p, p, None) != 0 and b"null pointer" in err()
    assert call(p, 2, p, None, 1.0, 1, 4, p, p, p, None) != 0 and b"layout = 2" in err()
    assert call(p, 0, p, None, 0.0, 1, 4, p, p, p, None) != 0 and b"temperature = 0" in err()
    assert call(p, 0, p, None, -1.0, 1, 4, p, p, p, None) != 0 and b"temperature = -1" in err()
    assert call(p, 0, p, None, float("nan"), 1, 4, p, p, p, None) != 0 and b"temperature" in err()
    assert call(p, 0, p, None, float("inf"), 1, 4, p, p, p, None) != 0 and b"temperature" in err()
    assert call(p, 0, p, None, 1.0, 0, 4, p, p, p, None) != 0 and b"F = 0" in err()
    assert call(p, 0, p, None, 1.0, 65536, 4, p, p, p, None) != 0 and b"F = 65536" in err()
    assert call(p, 0, p, None, 1.0, 1, 0, p, p, p, None) != 0 and b"L = 0" in err()
    assert call(p, 0, p, None, 1.0, 1, 4, None, None, None, None) != 0 and b"no output" in err()
    assert call(p, 0, p, None, 1.0, 1, 4, p, None, p, p) != 0 and b"frames sums the three per-location outputs" in err()
    assert call(p + 4, 1, p, None, 1.0, 1, 4, p, p, p, None) != 0 and b"aligned to 16 bytes" in err()
    t = torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        likelihood.code_nll(torch.zeros(1, 512, 4), t)
    with pytest.raises(ValueError, match="layout is 'hwc'"):
        likelihood.code_nll(torch.zeros(1, 512, 4), t, layout="hwc")
    with pytest.raises(ValueError, match="temperature = 0"):
        likelihood.code_nll(torch.zeros(1, 512, 4), t, temperature=0)


def test_result_type_arithmetic_on_a_hand_made_frames_table():
    #                         count  nll   entropy  hit
    frames = torch.tensor([[[6.0, 12.0, 3.0, 3.0], [2.0, 8.0, 4.0, 1.0]],       # frame 0: 6 observed, 2 sampled
                           [[8.0, 4.0, 16.0, 8.0], [0.0, 0.0, 0.0, 0.0]],       # frame 1: all observed -- its sampled group is empty
                           [[0.0, 0.0, 0.0, 0.0], [8.0, 24.0, 8.0, 2.0]]],      # frame 2: all sampled
                          dtype=torch.float64)
    r = likelihood.CodeNLL(None, None, None, frames)
    assert float(r.mean_nll("all")) == 48.0 / 24 and float(r.bits_per_code("all")) == pytest.approx(2.0 / LN2, rel=1e-15)
    assert float(r.bits_per_code("sampled")) == pytest.approx(32.0 / 10 / LN2, rel=1e-15)
    assert float(r.bits_per_code("observed")) == pytest.approx(16.0 / 14 / LN2, rel=1e-15)
    assert float(r.mean_entropy_bits("sampled")) == pytest.approx(1.2 / LN2, rel=1e-15)
    assert float(r.mean_entropy_bits("all")) == pytest.approx(31.0 / 24 / LN2, rel=1e-15)
    assert float(r.accuracy("sampled")) == 0.3 and float(r.accuracy("observed")) == 11.0 / 14 and float(r.accuracy("all")) == 14.0 / 24
    per = r.bits_per_code("sampled", per_frame=True)
    assert per.shape == (3,) and float(per[0]) == pytest.approx(4.0 / LN2) and math.isnan(float(per[1])) and float(per[2]) == pytest.approx(3.0 / LN2)
    assert math.isnan(float(r.accuracy("observed", per_frame=True)[2]))
    assert torch.equal(r.sums("all", per_frame=True)[:, 0], torch.tensor([8.0, 8.0, 8.0], dtype=torch.float64))
    # a batch without a sampled location: its sampled mean is NaN, the other groups are what they were
    alone = likelihood.CodeNLL(None, None, None, frames[1:2])
    assert math.isnan(float(alone.bits_per_code("sampled"))) and float(alone.mean_nll("all")) == float(alone.mean_nll("observed")) == 0.5
    with pytest.raises(ValueError, match="'background'"):
        r.bits_per_code("background")
    # what the driver writes from such a table
    rep = driver.validation_report(frames, ["a", "b", "c"], ["x", "y", "z"], [0, 1, 4])
    assert rep["count"] == 3 and [p["direction"] for p in rep["pairs"]] == ["R", "L", "UL"]
    assert rep["pairs"][1]["ar_bits_sampled"] is None and rep["pairs"][1]["n_sampled"] == 0 and rep["pairs"][2]["ar_bits_observed"] is None
    assert rep["pairs"][0]["autoreg_loss"] == 2.5 and rep["mean"]["autoreg_loss"] == 2.0 and rep["mean"]["ar_accuracy_sampled"] == 0.3
    assert rep["mean"]["n_sampled"] == 10 and rep["mean"]["n_observed"] == 14
    json.dumps(rep, allow_nan=False)


def test_driver_validate_argument_errors_come_before_any_device_is_touched(monkeypatch, tmp_path, capsys):
    from PIL import Image

    def touched(*a, **kw):
        raise AssertionError("the driver touched the device before it refused its arguments")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(driver, "build_model", touched)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    src, tgt, empty = tmp_path / "src", tmp_path / "tgt", tmp_path / "empty"
    for d, n in ((src, 2), (tgt, 3), (empty, 0)):
        d.mkdir()
        for i in range(n):
            Image.new("RGB", (8, 8)).save(d / f"{i}.png")
    out = str(tmp_path / "nll.json")
    dirs = str(tmp_path / "dirs.npy")
    np.save(dirs, np.array([0]))
    v = ["--validate", out]
    for argv, said in ((v + ["--image-dir", str(src)], "--validate needs --target-dir"),
                       (v + ["--target-dir", str(tgt)], "--validate needs --image ... or --image-dir"),
                       (v + ["--image-dir", str(src), "--target-dir", str(tgt), "--trajectory", "R"], "2 source images and 3 images in --target-dir"),
                       (v + ["--image-dir", str(src), "--target-dir", str(empty), "--trajectory", "R"], f"--target-dir {empty}: no "),
                       (v + ["--image-dir", str(src), "--target-dir", str(src)], "--trajectory R | L | U | D | UL | UR | DR | DL (got 'circle')"),
                       (v + ["--image-dir", str(src), "--target-dir", str(src), "--pairs", dirs], "holds 1 directions for 2 source images"),
                       (v + ["--image-dir", str(src), "--target-dir", str(src), "--scene", "R"], "--validate and --scene exclude each other"),
                       (v + ["--image-dir", str(src), "--target-dir", str(src), "--trajectory", "R", "--batch", "0"], "--batch must be >= 1"),
                       (["--image-dir", str(src), "--scene", "R", "--target-dir", str(tgt)], "--target-dir goes with --validate")):
        with pytest.raises(SystemExit) as exit_:
            driver.main(argv)
        assert exit_.value.code == 2 and said in capsys.readouterr().err, argv
    assert not (tmp_path / "nll.json").exists()
    # accepted arguments: the pairs and their directions, still without a device
    ap_error = lambda msg: (_ for _ in ()).throw(AssertionError(msg))
    import argparse
    args = argparse.Namespace(scene=None, num_samples=1, batch=4, target_dir=str(src), image=None, image_dir=str(src), pairs=None, trajectory="UL")
    sources, targets, ids = driver.validation_setup(args, ap_error)
    assert sources == targets == [str(src / "0.png"), str(src / "1.png")] and ids == [4, 4]
    np.save(dirs, np.array([3, 6]))
    args.pairs = dirs
    assert driver.validation_setup(args, ap_error)[2] == [3, 6]
