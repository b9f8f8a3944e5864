"""CPU: bench.py --dump-outputs keeps under its 64 MB cap -- arrays whole while they fit, otherwise the code grids whole and a
fixed, seeded sample of the views' images, the same rows for every array of the same length."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(V, seed):
    g = torch.Generator().manual_seed(seed)
    return {"codes": torch.randint(0, 512, (V, 32, 32), dtype=torch.int32, generator=g),
            "gen_fs": torch.rand(V, 3, 256, 256, generator=g),
            "background_mask": torch.rand(V, 256, 256, generator=g) > 0.5, "plan": None}


def _dump(tmp_path, tag, out):
    sys.path.insert(0, ROOT)
    import bench
    d = tmp_path / tag
    bench.dump_outputs(str(d), out)
    assert sum(p.stat().st_size for p in d.iterdir()) <= 64_000_000
    got = {p.stem: np.load(p) for p in d.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    return got


def test_small_batch_is_dumped_whole(tmp_path):
    out = _outputs(16, 0)
    got = _dump(tmp_path, "small", out)
    assert sorted(got) == ["background_mask", "background_mask_rows", "codes", "gen_fs", "gen_fs_rows"]
    assert np.array_equal(got["codes"], out["codes"].float().numpy())
    assert np.array_equal(got["gen_fs"], out["gen_fs"].numpy())
    assert np.array_equal(got["background_mask"], out["background_mask"].float().numpy())
    assert np.array_equal(got["gen_fs_rows"], np.arange(16))


def test_large_batch_is_sampled_the_same_way_every_time(tmp_path):
    out = _outputs(128, 1)
    got = _dump(tmp_path, "a", out)
    rows = got["gen_fs_rows"].astype(np.int64)
    assert 32 <= len(rows) < 128 and np.array_equal(rows, got["background_mask_rows"]) and (np.diff(rows) > 0).all()
    assert np.array_equal(got["codes"], out["codes"].float().numpy())              # the code grids whole
    assert np.array_equal(got["gen_fs"], out["gen_fs"].numpy()[rows])
    assert np.array_equal(got["background_mask"], out["background_mask"].float().numpy()[rows])
    again = _dump(tmp_path, "b", _outputs(128, 2))
    assert np.array_equal(again["gen_fs_rows"], got["gen_fs_rows"])                  # fixed rows, whatever the values
