"""CPU: the FID network (networks/inception.py) on its torch path against the fp64 restatement (tests/golden/fid_ref64.py, recorded in
tests/golden/fid.npz); its structure and state-dict keys; weight loading; BatchNorm folding and the packed weight layout of
include/pixelsynth_fid.h; the statistics and the Fréchet distance; the argument checks of inception_features and the CLI's
--inception checks, before any device is touched; the C ABI of the FID library.

The float bound of the network is 4 x err32, the restatement's own fp32 error against its fp64 run (two fp32 evaluations differ in
summation order only)."""
import json
import os

import numpy as np
import pytest
import torch

from abi_util import assert_library_matches_header
import fid_ref64 as R
from pixelsynth_amd import _lib, fid, synthetic as syn
from pixelsynth_amd.networks import inception as I



@pytest.fixture(scope="module")
def net():
    return I.FIDInception(weights={k: torch.from_numpy(v) for k, v in R.weights().items()})


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fid.npz"))


def test_golden_file_matches_its_inputs(golden):
    assert json.loads(str(golden["cases"])) == R.CASES and int(golden["weight_seed"]) == R.WEIGHT_SEED
    assert json.loads(str(golden["fid_sets"])) == R.FID_SETS
    for case in R.CASES:
        assert float(np.asarray(R.case_input(case), np.float64).sum()) == float(golden["sum/" + case[0]])
        f = golden["f64/" + case[0]]
        assert f.shape == (1, 2048) and f.dtype == np.float64
        assert f.std() > 0.5 and np.mean(f == 0) < 0.5, "features that do not vary test nothing"
        assert 0 < float(golden["err32/" + case[0]]) < 1e-3


def test_torch_path_against_the_fp64_restatement(net, golden):
    assert len(R.CASES) == 3 and sorted(c[3] for c in R.CASES) == [256, 299, 299]
    for case in R.CASES:
        with torch.no_grad():
            got = net.torch_forward(torch.from_numpy(R.case_input(case))).double().numpy()
        err, bound = np.abs(got - golden["f64/" + case[0]]).max(), 4 * float(golden["err32/" + case[0]])
        print(f"{case[0]}: torch fp32 vs fp64 {err:.3e} (bound {bound:.3e})")
        assert err <= bound, case[0]


def test_restatement_reproduces_its_record(golden):
    case = R.CASES[2]
    with torch.no_grad():
        f64 = R.features(R.weights(), R.case_input(case), torch.float64).numpy()
    assert np.abs(f64 - golden["f64/" + case[0]]).max() <= 1e-10


def test_structure_and_state_dict_keys(net, golden):
    specs = I.conv_specs()
    assert len(specs) == 94 and len([m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]) == 94
    assert str(golden["source"]) in ("pytorch_fid", "torchvision", "restated")
    skip = lambda k: k.endswith("num_batches_tracked")
    assert [[k, list(v.shape)] for k, v in net.state_dict().items() if not skip(k)] == json.loads(str(golden["state_keys"]))
    used = [n for _, branches in I.NETWORK for steps in branches for s in steps for n in (s if isinstance(s, tuple) else (s,))
            if n not in I.POOLS]
    assert sorted(used) == sorted(specs), "every convolution runs exactly once"
    with torch.no_grad():
        assert tuple(net(torch.rand(1, 3, 75, 91)).shape) == (1, 2048)


def test_weight_loading(net, tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in R.weights().items()}
    full = dict(sd)
    full["fc.weight"], full["fc.bias"], full["AuxLogits.conv0.conv.weight"] = torch.zeros(8, 2048), torch.zeros(8), torch.zeros(1)
    full["Mixed_5b.branch1x1.bn.num_batches_tracked"] = torch.tensor(0)
    path = str(tmp_path / "pt_inception-2015-12-05-6726825d.pth")
    torch.save(full, path)
    x = torch.from_numpy(R.case_input(["x", "blur", 5, 80, 96]))
    with torch.no_grad():
        want = net.torch_forward(x)
        for w in (path, full, net.state_dict()):
            assert torch.equal(I.FIDInception(weights=w).torch_forward(x), want)
    missing = {k: v for k, v in sd.items() if k != "Mixed_6c.branch7x7_2.bn.running_var"}
    with pytest.raises(KeyError, match="Mixed_6c.branch7x7_2.bn.running_var"):
        I.FIDInception(weights=missing)
    bad = dict(sd)
    bad["Mixed_7a.branch3x3_2.conv.weight"] = torch.zeros(320, 192, 3, 1)
    with pytest.raises(ValueError, match=r"Mixed_7a.branch3x3_2.conv.weight has shape \(320, 192, 3, 1\)"):
        I.FIDInception(weights=bad)
    with pytest.raises(KeyError, match="unexpected key Mixed_9z"):
        I.FIDInception(weights=dict(sd, **{"Mixed_9z.conv.weight": torch.zeros(1)}))


def test_synthetic_weights_exercise_the_folding():
    sd = R.weights()
    assert len(sd) == 94 * 5 and all(v.dtype == np.float32 for v in sd.values())
    g, v = sd["Mixed_6e.branch7x7dbl_3.bn.weight"], sd["Mixed_6e.branch7x7dbl_3.bn.running_var"]
    assert 0.5 <= g.min() < 0.7 and 1.3 < g.max() <= 1.5 and 0.5 <= v.min() < 0.7 and 1.3 < v.max() <= 1.5
    assert np.array_equal(syn.inception_state_dict(3)["Conv2d_1a_3x3.conv.weight"], syn.inception_state_dict(3)["Conv2d_1a_3x3.conv.weight"])


def test_folded_convolution_is_the_conv_bn_pair(net):
    name = "Mixed_6c.branch7x7dbl_2"
    ci, co, k, s, p = I.conv_specs()[name]
    x = torch.randn(1, ci, 9, 9, dtype=torch.float64)
    w, b = net.folded(name)
    assert w.dtype == torch.float32 and b.dtype == torch.float32
    m = net.conv(name).double()
    try:
        with torch.no_grad():
            want = m(x)
    finally:
        m.float()
    got = torch.relu(torch.nn.functional.conv2d(x, w.double(), b.double(), s, p))
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())      # fp32 rounding of w', b' only


def test_packed_weight_layout_is_the_header_formula():
    rs = np.random.RandomState(4)
    for co, ci, kh, kw in ((80, 12, 1, 3), (64, 3, 3, 3), (20, 20, 2, 1), (37, 8, 1, 1)):
        w = torch.from_numpy(rs.randn(co, ci, kh, kw).astype(np.float32))
        layer = fid.pack_conv(w, torch.zeros(co), 1, (0, 0))
        cp = (ci + 3) // 4 * 4
        assert layer["Ci"] == cp and layer["Co"] == co
        T = _lib.call("ps_fid_conv_co_tile", co)
        assert T == (32 if co in (80, 20) else 64)
        K = kh * kw * cp
        S = (K + 63) // 64
        w2 = np.zeros(((co + T - 1) // T * T, S * 64), np.float32)
        wk = np.zeros((co, kh, kw, cp), np.float32)
        wk[..., :ci] = w.numpy().transpose(0, 2, 3, 1)
        w2[:co, :K] = wk.reshape(co, K)
        wp = layer["wp"].numpy()
        assert wp.size == w2.size == _lib.call("ps_fid_conv_packed_floats", kh, kw, cp, co)
        idx = rs.randint(0, wp.size, 4000)
        for e in idx:
            j, i, kk, t, c = e % 4, e // 4 % 16, e // 64 % 4, e // 256 % (T // 16), e // (256 * (T // 16)) % 4
            s, cb = e // (1024 * (T // 16)) % S, e // (1024 * (T // 16) * S)
            assert wp[e] == w2[cb * T + 16 * t + i, 64 * s + 16 * c + 4 * kk + j]
    assert fid.pack_conv(torch.zeros(8, 4, 9, 1), torch.zeros(8)) is None            # outside what the kernel takes: the caller falls back
    assert not _lib.call("ps_fid_conv_takes", 3, 3, 3, 1, 1, 16, 16) and not _lib.call("ps_fid_conv_takes", 3, 3, 1, 1, 1, 6, 16)
    assert _lib.call("ps_fid_conv_takes", 7, 1, 2, 3, 0, 4, 1)


def _spd(rs, d, n):
    rows = rs.randn(n, d) @ rs.randn(d, d) + rs.randn(d)
    return rows


def test_statistics_against_numpy():
    rs = np.random.RandomState(7)
    rows = _spd(rs, 24, 100)
    mu, sigma = fid.statistics(rows.astype(np.float32))
    r64 = rows.astype(np.float32).astype(np.float64)
    assert mu.dtype == torch.float64 and sigma.dtype == torch.float64
    np.testing.assert_allclose(mu.numpy(), r64.mean(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sigma.numpy(), np.cov(r64, rowvar=False), rtol=1e-11, atol=1e-11)
    with pytest.raises(ValueError, match="N >= 2"):
        fid.statistics(rows[:1])


def test_frechet_distance_properties():
    rs = np.random.RandomState(8)
    mu, sigma = fid.statistics(_spd(rs, 64, 512))
    assert abs(fid.frechet_distance(mu, sigma, mu, sigma)) <= 1e-9 * 2 * float(torch.trace(sigma))
    # diagonal covariances: the closed form
    a, b, m1, m2 = rs.rand(40) + 0.1, rs.rand(40) + 0.1, rs.randn(40), rs.randn(40)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((m1 - m2) ** 2).sum()
    assert abs(fid.frechet_distance(m1, np.diag(a), m2, np.diag(b)) - want) <= 1e-10 * want
    # random SPD pairs against numpy's eigenvalues of the plain product
    for d in (8, 16, 33, 64):
        (m1, s1), (m2, s2) = (fid.statistics(_spd(rs, d, 4 * d)) for _ in range(2))
        tr = np.sqrt(np.linalg.eigvals(s1.numpy() @ s2.numpy()).real.clip(0)).sum()
        want = float(((m1 - m2) ** 2).sum() + torch.trace(s1) + torch.trace(s2) - 2 * tr)
        got = fid.frechet_distance(m1, s1, m2, s2)
        assert abs(got - want) <= 1e-9 * (float(torch.trace(s1)) + float(torch.trace(s2))), d
        assert abs(got - fid.frechet_distance(m2, s2, m1, s1)) <= 1e-9 * (float(torch.trace(s1)) + float(torch.trace(s2))), d
    # singular covariances (fewer rows than dimensions): finite and >= 0
    r1, r2 = _spd(rs, 48, 10), _spd(rs, 48, 12)
    got = fid.fid_of_rows(r1, r2)
    assert np.isfinite(got) and got >= 0
    assert abs(got - R.fid64(r1, r2)) <= 1e-6 * got
    with pytest.raises(ValueError, match="one D"):
        fid.frechet_distance(np.zeros(3), np.eye(3), np.zeros(3), np.eye(4))


def test_inception_features_argument_checks(net):
    a = torch.zeros(2, 3, 64, 64)
    with pytest.raises(ValueError, match=r"\(B, 3, H, W\)"):
        fid.inception_features(net, a[0])
    with pytest.raises(ValueError, match="C must be 3"):
        fid.inception_features(net, torch.zeros(2, 1, 8, 8))
    with pytest.raises(TypeError, match="float32 or uint8"):
        fid.inception_features(net, a.double())
    with pytest.raises(TypeError, match="FIDInception"):
        fid.inception_features(object(), a)
    with pytest.raises(TypeError, match="tensor"):
        fid.inception_features(net, a.numpy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fid.inception_features(net, a)
    assert 64 <= fid.images_per_pass() <= 256


def test_cli_inception_argument_errors(tmp_path, capsys):
    from pixelsynth_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--pred", str(tmp_path), "--gt", str(tmp_path), "--inception", str(tmp_path / "nope.pth")])
    assert e.value.code == 2 and "nope.pth" in capsys.readouterr().err
    weights = tmp_path / "w.pth"
    weights.write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--consistency", str(tmp_path), "--masks", str(tmp_path), "--points", str(tmp_path), "--directions",
                       str(tmp_path / "d.npy"), "--inception", str(weights)])
    assert e.value.code == 2 and "--inception" in capsys.readouterr().err


def test_fid_library_exports_its_header():
    assert_library_matches_header("fid")
    L = _lib.library("fid")
    with pytest.raises(RuntimeError, match="ps_fid_pool failed.*null"):
        _lib.call("ps_fid_pool", None, 4, 0, 1, 8, 8, 4, None, 4, 0, stream=0)
    with pytest.raises(RuntimeError, match="ps_fid_conv failed.*null"):
        _lib.call("ps_fid_conv", None, 4, None, 0, None, 1, 8, 8, 4, 3, 3, 1, 1, 1, 8, None, 8, 0, stream=0)
    assert L.ps_fid_last_error()
