"""CPU-only: the host side of the batched chained scenes -- the driver's per-scene writers, its --pairs layout against what
evaluate --consistency lists, the directions file and flags, the deal of scenes over ranks -- on fake tensors, no device; and the C ABI
of libpixelsynth_scene.so against its header and bindings."""
import os

import numpy as np
import pytest
import torch

from abi_util import assert_library_matches_header
from pixelsynth_amd import _lib, driver, evaluate

S = 16


def _fake_pairs(B, names):
    g = torch.Generator().manual_seed(0)
    out = {"InputImg": torch.rand(B, 3, S, S, generator=g) * 2 - 1}
    for n in set(names):
        for i in (0, 1, 2):
            out[f"PredImg_{n}_{i}"] = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    return out


def test_pairs_writer_produces_what_consistency_discover_lists(tmp_path):
    """--pairs writes <out>/<%04d>/{input_image_, output_image_<d>_0001, output_image_<d>_0002}.png (eval_consistency.py:122-149);
    with stand-in mask and point files in place, evaluate.consistency_discover finds every item's views."""
    from PIL import Image
    ids = [0, 1, 2, 5, 7, 3]
    views, masks, points = (str(tmp_path / d) for d in ("views", "masks", "points"))
    os.makedirs(points)
    np.save(str(tmp_path / "directions.npy"), np.asarray(ids))
    # two groups, as two ranks or two batches would write them
    for group in ([0, 2, 4], [1, 3, 5]):
        gid = [ids[i] for i in group]
        driver.pairs_to_disk(_fake_pairs(len(group), [driver.MAPPING[d] for d in gid]), group, gid, views)
    for i in range(len(ids)):
        os.makedirs(os.path.join(masks, "%04d" % i))
        for k in (1, 2):
            Image.fromarray(np.zeros((S, S), np.uint8)).save(os.path.join(masks, "%04d" % i, f"mask{k}.png"))
            np.save(os.path.join(points, f"reproj{k}_{i}.npy"), np.zeros((4, 2), np.float32))
    items = evaluate.consistency_discover(views, masks, points, str(tmp_path / "directions.npy"))
    assert [it[0] for it in items] == list(range(len(ids)))
    for i, it in enumerate(items):
        d = driver.MAPPING[ids[i]]
        assert it[1].endswith(os.path.join("%04d" % i, f"output_image_{d}_0001.png")) and it[2].endswith(f"output_image_{d}_0002.png")
        assert sorted(os.listdir(os.path.join(views, "%04d" % i))) == ["input_image_.png", f"output_image_{d}_0001.png", f"output_image_{d}_0002.png"]
    # a missing view is still an error there: the writer is what makes the list complete
    os.remove(items[3][2])
    with pytest.raises(FileNotFoundError, match="item 3"):
        evaluate.consistency_discover(views, masks, points, str(tmp_path / "directions.npy"))


def test_pairs_writer_saves_the_scenes_own_slice(tmp_path):
    from PIL import Image
    out = _fake_pairs(2, ["R", "UR"])
    driver.pairs_to_disk(out, [4, 9], [0, 5], str(tmp_path))
    for b, (index, name) in enumerate(((4, "R"), (9, "UR"))):
        for i in (1, 2):
            got = np.asarray(Image.open(tmp_path / ("%04d" % index) / ("output_image_%s_%04d.png" % (name, i))))
            want = driver.D.to_image_u8(out[f"PredImg_{name}_{i}"][b]).permute(1, 2, 0).numpy()
            assert np.array_equal(got, want)
        got = np.asarray(Image.open(tmp_path / ("%04d" % index) / "input_image_.png"))
        assert np.array_equal(got, driver.D.to_image_u8(out["InputImg"][b]).permute(1, 2, 0).numpy())


def test_per_scene_writer_keeps_the_scene_layout_inside_every_scene_directory(tmp_path):
    """Scene b of a batch goes to <out>/<%04d>/ in exactly the files scene_outputs_to_disk writes for a B = 1 run of that scene."""
    directions, num_split, B = ["R", "L"], 2, 3
    g = torch.Generator().manual_seed(1)
    outputs = {f"PredImg_{d}_{i}": torch.rand(B, 3, S, S, generator=g) * 2 - 1 for d in directions for i in range(num_split + 1)}
    outputs["FeaturesImg_R_0"] = torch.zeros(B, 3, S, S)
    group = [7, 2, 11]
    n = driver.scenes_to_disk(outputs, group, directions, num_split, str(tmp_path / "batched"))
    for b, index in enumerate(group):
        one = {k: v[b:b + 1] for k, v in outputs.items()}
        alone = str(tmp_path / "alone" / str(index))
        assert driver.scene_outputs_to_disk(one, directions, num_split, alone) == n
        for sub in ("scene", "video"):
            here = os.path.join(driver.scene_dir(str(tmp_path / "batched"), index), sub)
            assert sorted(os.listdir(here)) == sorted(os.listdir(os.path.join(alone, sub))) != []
            for f in os.listdir(here):
                assert open(os.path.join(here, f), "rb").read() == open(os.path.join(alone, sub, f), "rb").read(), (index, sub, f)
    assert sorted(os.listdir(tmp_path / "batched")) == ["0002", "0007", "0011"]


def test_directions_file_and_flags(tmp_path):
    good = str(tmp_path / "d.npy")
    np.save(good, np.asarray([0, 7, 3, 1]))
    assert driver.load_directions(good, 3) == [0, 7, 3]
    with pytest.raises(ValueError, match="holds 4 directions for 5 source images"):
        driver.load_directions(good, 5)
    np.save(str(tmp_path / "bad.npy"), np.asarray([0, 8]))
    with pytest.raises(ValueError, match=r"item 1: direction 8 outside 0 \.\. 7"):
        driver.load_directions(str(tmp_path / "bad.npy"), 2)
    np.save(str(tmp_path / "2d.npy"), np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError, match="1-D array"):
        driver.load_directions(str(tmp_path / "2d.npy"), 2)
    assert driver.MAPPING == tuple(evaluate.CS.MAPPING)
    # sources: several --image paths, or a directory in sorted order; not both
    d = tmp_path / "imgs"
    d.mkdir()
    for f in ("b.png", "a.jpg", "notes.txt", "c.JPEG"):
        (d / f).write_bytes(b"")
    assert [os.path.basename(p) for p in driver.source_images(None, str(d))] == ["a.jpg", "b.png", "c.JPEG"]
    assert driver.source_images(["x.png", "y.png"], None) == ["x.png", "y.png"] and driver.source_images(None, None) == []
    with pytest.raises(ValueError, match="exclude each other"):
        driver.source_images(["x.png"], str(d))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no .png"):
        driver.source_images(None, str(tmp_path / "empty"))
    # flag combinations main() refuses before it touches a device
    for argv in (["--image", "a.png", "b.png"], ["--image-dir", str(d)], ["--scene", "R", "--pairs", good, "--image", "a.png"], ["--pairs", good]):
        with pytest.raises(SystemExit):
            driver.main(argv)


@pytest.mark.parametrize("n,batch,world", [(10, 3, 4), (3600, 16, 8), (5, 16, 1), (3, 2, 8), (0, 4, 2)])
def test_scenes_are_dealt_over_ranks_without_loss_or_duplication(n, batch, world):
    seen = []
    for rank in range(world):
        groups = driver.scene_groups(n, batch, rank, world)
        assert all(1 <= len(g) <= batch for g in groups)
        mine = [i for g in groups for i in g]
        assert mine == driver.D.shard_views(n, rank, world)
        seen += mine
    assert sorted(seen) == list(range(n))
    with pytest.raises(ValueError, match="--batch"):
        driver.scene_groups(n, 0, 0, world)


def test_scene_library_exports_what_its_header_declares():
    """include/pixelsynth_scene.h, the exports of libpixelsynth_scene.so and _lib.SCENE_PROTOS name the same entry points with the same
    number of parameters; libpixelsynth_hip.so's ABI is untouched (tests/test_abi.py) and its version stays 2."""
    protos = assert_library_matches_header("scene")
    assert set(protos) == set(_lib.SCENE_PROTOS) and len(protos) == 4
    assert _lib.call("ps_abi_version") == 2


def test_scene_size_queries_are_host_arithmetic():
    B, C, cap, S_ = 4, 3, 3 * 256 * 256, 256
    assert _lib.call("ps_scene_state_bytes", B, C, cap) == (2 * 4 + 2 * C) * 4 * cap * B + 4 * B
    assert _lib.call("ps_scene_state_bytes", 0, C, cap) == 0 and _lib.call("ps_scene_workspace_bytes", B, 0, S_, 4.0) == 0
    ws, splat = _lib.call("ps_scene_workspace_bytes", B, cap, S_, 4.0), _lib.call("ps_splat_workspace_bytes", B, cap, S_, 4.0)
    assert splat < ws <= splat + 4 * B * (S_ * S_ // 256 + 1) + 256   # the splat's for clouds of cap points + the compaction's block sums
    # refused on the host before anything is enqueued (no stream is touched: NULL pointers fail first)
    L = _lib.library("scene")
    assert L.ps_scene_step_f32(*([None] * 13), 1, 3, 16, 256, 0, 256, 4.0, 8, 1.0, 2, 0, 13, None, None, None, 0, None) < 0
    assert b"null pointer" in L.ps_scene_last_error()
