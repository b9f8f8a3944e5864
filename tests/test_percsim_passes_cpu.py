"""No GPU: the fp64 reference of tests/_percsim_pass_cases.py against the torch formula of networks/pretrained_networks.py in float64,
and the conditions on the cases that tests/test_percsim_passes_gpu.py rests on, so that they cannot quietly stop testing what they
are for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _percsim_pass_cases as E
from pixelsynth_amd.networks.pretrained_networks import cos_sim

# the cheap cases: the two smallest sizes with P = 3, on and off the network's channels (every case is looked at below, by shape)
SMALL = [k for k, c in enumerate(E.CASES) if c[:3] in ((128, 128, 3), (256, 128, 1))]


def nchw(y):
    return torch.from_numpy(np.array(y)).double().permute(0, 3, 1, 2)


@pytest.mark.parametrize("k", SMALL, ids=[E.name(E.CASES[k]) for k in SMALL])
@pytest.mark.parametrize("maps_of", [E.integer_maps, E.float_maps], ids=["integer", "float"])
def test_reference_is_the_torch_formula_in_float64(k, maps_of):
    P, maps = E.CASES[k][2], maps_of(k)
    layers, total = E.scores64(maps, P)
    want = np.ones((P, E.LAYERS))
    for l, y in maps.items():
        x = torch.relu(nchw(y))
        want[:, l] = (1.0 - cos_sim(x[:P], x[P:])).numpy()
        assert np.abs(E.tap64(y, P) - (1.0 - want[:, l])).max() <= 1e-12
        assert torch.equal(nchw(E.pool(y)), F.max_pool2d(nchw(y), 2, 2)), "pool is max_pool2d of the raw map"
    assert np.abs(layers - want).max() <= 1e-12 and np.abs(total - want.sum(1)).max() <= 1e-12
    assert set(range(E.LAYERS)) - set(maps) == set(np.flatnonzero((layers == 1.0).all(0))), "an untapped layer scores exactly 1"


@pytest.mark.parametrize("k", range(len(E.CASES)), ids=[E.name(c) for c in E.CASES])
def test_every_integer_case_holds_every_forced_pixel(k):
    case = E.CASES[k]
    P = case[2]
    for l, y in E.integer_maps(k).items():
        assert y.shape == E.map_shape(case, l) and np.abs(y).max() == 3 and np.array_equal(y, np.round(y))
        assert 0.55 <= (y < 0).mean() <= 0.65
        n = E.norms64(y)
        assert (n == 0).mean((1, 2)).max() <= 1 / 8, "zero-norm pixels are a small part of every map"
        spots = E.forced_spots(case, l)
        for pair in range(P):
            y0, y1, n0, n1 = y[pair], y[P + pair], n[pair], n[P + pair]
            s = spots[pair]
            assert n0[s["in0_zero"]] == 0 and n1[s["in0_zero"]] > 0, "all channels <= 0 in in0 only"
            assert n1[s["in1_zero"]] == 0 and n0[s["in1_zero"]] > 0, "all channels <= 0 in in1 only"
            assert n0[s["both_zero"]] == 0 and n1[s["both_zero"]] == 0, "all channels <= 0 in both"
            assert n0[s["equal"]] > 0 and np.array_equal(y0[s["equal"]], y1[s["equal"]]), "a pixel where in0 == in1"
            r, c = s["negative_window"]
            ch = (7 * pair + 5) % y.shape[3]
            for img in (y0, y1):
                assert (img[r:r + 2, c:c + 2, ch] < 0).all() and r % 2 == 0 and c % 2 == 0, "a pool window all negative in a channel"
        # the sign convention of the pool decides the expected map
        raw, post = E.pool(y), E.pool(y, relu_first=True)
        assert (raw < 0).any() and not np.array_equal(raw, post)
        assert np.array_equal(np.maximum(raw, 0), post), "relu(max(y)) = max(relu(y)): the next convolution cannot tell"


def test_the_cases_reach_the_shapes_they_are_for():
    assert [c[:2] for c in E.NET_CASES[::2]] == [(128, 128), (128, 384), (384, 128), (256, 128)] and {c[2] for c in E.CASES} == {1, 3}
    assert all(c[3] == {0: 64, 1: 128, 2: 256, 3: 512, 4: 512} for c in E.NET_CASES)
    off = {(l, ch) for c in E.OFF_CASES for l, ch in c[3].items()}
    assert off == {(3, 192), (3, 320), (4, 192), (4, 320)}, "C = 192 and 320 at layers 3 and 4 only"
    assert {c[:3] for c in E.OFF_CASES} == {c[:3] for c in E.NET_CASES}
    shapes = [(case, l) for case in E.CASES for l in case[3]]
    tiles = {E.tiles_of(case[0], case[1], l) for case, l in shapes}
    assert 1 in tiles and max(tiles) > 64, tiles
    assert any(16 % ((case[1] >> l) // 2) for case, l in shapes), "a tile that straddles a map row"
    assert (128 >> 4, 384 >> 4) == (8, 24) and E.tiles_of(128, 384, 4) == 3, "the 8 x 24 map: Wq = 12, three tiles"
    # maps that are not square, whose width is no power of two, narrower than a tile, and lane-loop trip counts 1 .. 8 with 3 and 5
    assert {case[3][l] // 64 for case, l in shapes} == {1, 2, 3, 4, 5, 8}
    assert any((case[1] >> l) // 2 < 16 for case, l in shapes) and any((case[1] >> l) // 2 > 16 for case, l in shapes)
    # what the finish test asks of its sizes
    assert {E.tiles_of(128, 128, 0), E.tiles_of(128, 128, 4), E.tiles_of(128, 384, 0), E.tiles_of(128, 384, 4)} == {256, 1, 768, 3}
    for P, H, W in ((1, 128, 128), (3, 128, 384), (65535, 384, 128)):
        assert E.workspace_bytes(P, H, W) == 8 * E.layer_offset(P, H, W, 5) == 8 * P * (H * W // 64) * 341 // 256


@pytest.mark.parametrize("maps_of", [E.integer_maps, E.float_maps], ids=["integer", "float"])
def test_the_images_of_a_pass_are_all_different(maps_of):
    """Swapping in0 and in1's places across pairs (P + i read as i, or pair i's in1 as pair j's) moves every expected score by far
    more than any bound of the GPU tests"""
    k = E.CASES.index((128, 128, 3, dict(enumerate(E.NET_C))))
    P, maps = 3, maps_of(k)
    layers, _ = E.scores64(maps, P)
    for l, y in maps.items():
        assert len({y[i].tobytes() for i in range(2 * P)}) == 2 * P
        rolled = np.concatenate([y[:P], np.roll(y[P:], 1, 0)])            # pair i against pair i - 1's in1
        same = np.concatenate([y[:P], y[:P]])                             # off1 read from `pair`: in0 against itself
        for wrong in (rolled, same):
            assert np.abs((1.0 - E.tap64(wrong, P)) - layers[:, l]).min() > 1e-2, l
    if maps_of is E.float_maps:
        assert all((y != 0).all() for y in maps.values()), "no exact zero"
        assert all(abs(float(y.mean()) + 0.3) < 0.01 and abs(float(y.std()) - 1) < 0.01 for y in maps.values())


def test_rounding_bound_and_finish_reference():
    assert E.rounding_bound(512) == 75 * 2.0 ** -24 and 4.4e-6 < E.rounding_bound(512) < 4.5e-6
    assert [E.rounding_bound(C) * 2 ** 24 for C in (64, 128, 192, 256, 320)] == [19, 27, 35, 43, 51]
    for P, H, W in ((3, 128, 128), (3, 128, 384)):
        ws = E.finish_workspace(P, H, W)
        assert len(np.unique(ws)) == len(ws) == E.workspace_bytes(P, H, W) // 8 and np.array_equal(ws * 4096, np.round(ws * 4096))
        layers, total = E.finish64(ws, P, H, W)
        assert layers.dtype == total.dtype == np.float32 and ((layers > 0) & (layers < 1)).all()
        assert np.abs(total - layers.astype(np.float64).sum(1)).max() <= 2.0 ** -21
        assert len(np.unique(layers)) == layers.size, "no two (pair, layer) sums coincide: a misplaced block shows"
