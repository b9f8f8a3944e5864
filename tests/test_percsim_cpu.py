"""CPU: PercSim's network (networks/pretrained_networks.py) on its torch path against the reference's outputs (tests/golden/percsim.npz)
and the fp64 restatement (tests/golden/percsim_ref64.py); state-dict keys; weight loading and where the default weights are looked for;
the argument checks of perceptual_rows and the CLI's --vgg16 check, before any device is touched; the C ABI of the PercSim library."""
import json
import os
import re

import numpy as np
import pytest
import torch

from abi_util import assert_library_matches_header
import percsim_ref64 as R
from pixelsynth_amd import _lib, synthetic as syn
from pixelsynth_amd.networks.pretrained_networks import PNet, cos_sim, normalize_tensor
from pixelsynth_amd.perceptual import perceptual_rows

MARGIN = 1e-7      # beyond the reference's own recorded fp32 error: a different order of fp32 sums


@pytest.fixture(scope="module")
def net():
    sd = {k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(R.WEIGHT_SEED).items()}
    return PNet(use_gpu=False, weights=sd)


def rows_of(net, x0, x1):
    with torch.no_grad():
        val, layers = net(torch.from_numpy(x0) * 2 - 1, torch.from_numpy(x1) * 2 - 1, retPerLayer=True)
    return np.concatenate([torch.stack(layers, 1).numpy(), val.numpy()[:, None]], 1).astype(np.float64)


def test_golden_file_matches_its_inputs(golden_dir):
    z = np.load(os.path.join(golden_dir, "percsim.npz"))
    assert json.loads(str(z["cases"])) == [list(c) for c in R.CASES] and int(z["weight_seed"]) == R.WEIGHT_SEED
    for case in R.CASES:
        a, b, m = R.case_inputs(case)
        assert float(sum(np.asarray(x, np.float64).sum() for x in (a, b, m) if x is not None)) == float(z["sum/" + case[0]])
        assert z["ref/" + case[0]].shape == (1 if m is None else 3, case[2], 6)


def test_torch_path_and_fp64_against_reference(net, golden_dir):
    z = np.load(os.path.join(golden_dir, "percsim.npz"))
    for case in R.CASES:
        a, b, m = R.case_inputs(case)
        ref, err32 = z["ref/" + case[0]].astype(np.float64), z["err32/" + case[0]]
        got = np.stack([rows_of(net, x0, x1) for x0, x1 in R.variants(a, b, m)])
        assert (np.abs(got - ref).max((0, 1)) <= 2 * err32 + MARGIN).all(), case[0]
        r64 = R.case64(case)
        assert (np.abs(r64 - ref).max((0, 1)) <= err32 * (1 + 1e-9)).all(), case[0]


def test_state_dict_keys_equal_the_reference(net, golden_dir):
    z = np.load(os.path.join(golden_dir, "percsim.npz"))
    want = json.loads(str(z["state_keys"]))
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want
    assert want[0][0] == "net.slice1.0.weight" and want[-1][0] == "net.slice5.28.bias"


def test_weight_formats_give_identical_outputs(net, tmp_path):
    tv = {k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(R.WEIGHT_SEED).items()}
    tv["classifier.0.weight"], tv["classifier.0.bias"] = torch.zeros(8, 4), torch.zeros(8)     # ignored
    path = str(tmp_path / "vgg16.pth")
    torch.save(tv, path)
    own = str(tmp_path / "pnet.pth")
    torch.save(net.state_dict(), own)
    a, b = syn.metric_pair(41, 1, 3, 32, 48)
    want = rows_of(net, a, b)
    for w in (path, own, net.state_dict()):
        assert np.array_equal(rows_of(PNet(use_gpu=False, weights=w), a, b), want)


def test_default_weights_in_torch_home(tmp_path, monkeypatch):
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    path = os.path.join(str(tmp_path), "hub", "checkpoints", "vgg16-397923af.pth")
    with pytest.raises(FileNotFoundError, match=re.escape(path) + ".*weights="):
        PNet(use_gpu=False)
    os.makedirs(os.path.dirname(path))
    torch.save({k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(3).items()}, path)
    net = PNet(use_gpu=False)
    assert torch.equal(net.net.slice1[0].weight, torch.from_numpy(syn.vgg16_state_dict(3)["features.0.weight"]))
    rand = PNet(use_gpu=False, pnet_rand=True)           # torchvision's initialisation, no file needed
    assert float(rand.net.slice1[0].bias.abs().max()) == 0.0
    assert "shift" not in dict(net.state_dict()) and "scale" not in dict(net.state_dict())
    for kind in ("alex", "squeeze", "resnet18", "resnet50"):
        with pytest.raises(NotImplementedError):
            PNet(pnet_type=kind, use_gpu=False)


def test_cos_sim_of_identical_maps_is_one():
    x = torch.rand(2, 8, 5, 7)
    torch.testing.assert_close(cos_sim(x, x), torch.ones(2), rtol=0, atol=1e-6)
    n = normalize_tensor(x)
    torch.testing.assert_close(n.pow(2).sum(1), torch.ones(2, 5, 7), rtol=0, atol=1e-5)


def test_perceptual_rows_argument_checks(net):
    a = torch.zeros(2, 3, 256, 256)
    with pytest.raises(ValueError, match="differ in shape"):
        perceptual_rows(net, a, torch.zeros(2, 3, 256, 128))
    with pytest.raises(ValueError, match=r"\(B, 3, H, W\)"):
        perceptual_rows(net, a[0], a[0])
    with pytest.raises(ValueError, match="C must be 3"):
        perceptual_rows(net, torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    with pytest.raises(TypeError, match="float32 or both uint8"):
        perceptual_rows(net, a.double(), a.double())
    with pytest.raises(ValueError, match="mask must be"):
        perceptual_rows(net, a, a, torch.zeros(2, 3, 256, 256))
    with pytest.raises(TypeError, match="PNet"):
        perceptual_rows(object(), a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        perceptual_rows(net, a, a)


def test_cli_rejects_a_missing_vgg16_file(tmp_path, capsys):
    from pixelsynth_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--pred", str(tmp_path), "--gt", str(tmp_path), "--vgg16", str(tmp_path / "nope.pth")])
    assert e.value.code == 2 and "nope.pth" in capsys.readouterr().err


def test_percsim_library_exports_its_header():
    assert_library_matches_header("percsim")
    L = _lib.library("percsim")
    assert _lib.call("ps_percsim_workspace_bytes", 2, 256, 256) == 2 * (1024 + 256 + 64 + 16 + 4) * 8
    assert _lib.call("ps_percsim_workspace_bytes", 2, 96, 160) == 0
    with pytest.raises(RuntimeError, match="ps_percsim_finish failed.*null"):
        _lib.call("ps_percsim_finish", None, 0, 1, 256, 256, None, None, stream=0)
    assert L.ps_percsim_last_error()
