"""Cases the tests of PercSim's three passes share (tests/test_percsim_passes_cpu.py on the cases and the reference alone,
tests/test_percsim_passes_gpu.py on ps_percsim_input, ps_percsim_tap and ps_percsim_finish of csrc/percsim.hip), and the fp64 reference
of the tap and the finish.  Plain numpy on the CPU; nothing here touches a device or the network.

k_percsim_tap walks a map of (H >> l) x (W >> l) pixels in quads (2 x 2 pixel blocks, Wq = (W >> l) / 2 a row) and tiles of 16
consecutive quads, 16 lanes a quad, a lane 4 channels of every 64; k_percsim_finish adds a pair's tiles over 64 lanes.  The image sizes
are the smallest the ABI takes and the ones whose maps are not square or no power of two: at layer 4 a 128 x 384 image is an 8 x 24
map, Wq = 12, and tile 0 is all of quad row 0 and a third of row 1."""
import functools

import numpy as np

LAYERS = 5
SIZES = [(128, 128), (128, 384), (384, 128), (256, 128)]
PAIRS = [1, 3]
NET_C = (64, 128, 256, 512, 512)                 # VGG16's channels at the five taps
# off the network, at layers 3 and 4 alone (maps of 16 x 16 and smaller ... 48 x 16): lane-loop trip counts of 3 and 5
OFF_C = [{3: 192, 4: 320}, {3: 320, 4: 192}]
# (H, W, P, {layer: C}): a pass taps the layers of the dict; the others keep a zero workspace block
NET_CASES = [(H, W, P, dict(enumerate(NET_C))) for H, W in SIZES for P in PAIRS]
OFF_CASES = [(H, W, P, chans) for H, W in SIZES for P in PAIRS for chans in OFF_C]
CASES = NET_CASES + OFF_CASES
KINDS = ("in0_zero", "in1_zero", "both_zero", "equal", "negative_window")
_VALUES = np.arange(-3, 4)
_WEIGHTS = np.array([0.2, 0.2, 0.2, 0.1, 0.1, 0.1, 0.1])       # 60 % negative, 10 % zero


def name(case):
    H, W, P, chans = case
    return f"{H}x{W}-P{P}-" + "_".join(f"l{l}c{c}" for l, c in sorted(chans.items())) if len(chans) < LAYERS else f"{H}x{W}-P{P}-net"


def map_shape(case, layer):
    H, W, P, chans = case
    return (2 * P, H >> layer, W >> layer, chans[layer])


def tiles_of(H, W, layer):
    return ((H >> layer) // 2) * ((W >> layer) // 2) // 16


def workspace_bytes(P, H, W):
    """ps_percsim_workspace_bytes in closed form: doubles [layer][pair][tile]"""
    return 8 * P * sum(tiles_of(H, W, l) for l in range(LAYERS))


def layer_offset(P, H, W, layer):
    """doubles in front of `layer`'s block"""
    return P * sum(tiles_of(H, W, l) for l in range(layer))


def _seed(case, salt):
    H, W, P, chans = case
    return [salt, H, W, P] + [c for _, c in sorted(chans.items())]


def forced_spots(case, layer):
    """Per pair, where integer_maps forces its pixels: five different quads of the map, a pixel in each of the first four ->
    {pair: {kind: (row, col)}}; the window's entry is its top left pixel.  The channel of the window is (7 pair + 5) % C."""
    _, Hl, Wl, _ = map_shape(case, layer)
    rng = np.random.default_rng(_seed(case, 7000 + layer))
    out = {}
    for pair in range(case[2]):
        quads = rng.permutation((Hl // 2) * (Wl // 2))[:5]
        spot = {}
        for kind, q in zip(KINDS, quads):
            qy, qx = divmod(int(q), Wl // 2)
            dy, dx = (0, 0) if kind == "negative_window" else (int(rng.integers(2)), int(rng.integers(2)))
            spot[kind] = (2 * qy + dy, 2 * qx + dx)
        out[pair] = spot
    return out


def _share_pixels(y, P, rng):
    """Independent draws alone give every pairing of two images nearly the same mean cosine (they differ by the sampling noise of
    the map, 1e-3 and less): a pass that read pair j's in1 for pair i would move the scores by little.  So in1 of pair i takes in0's
    vector at (i + 1) / 8 of the pixels: the pairs' scores then lie about 0.1 apart, and the 2P images are still all different."""
    for pair in range(P):
        same = rng.random(y.shape[1:3]) < (pair + 1) / 8
        y[P + pair][same] = y[pair][same]


def _non_positive(v):
    return -np.abs(v) + np.float32(0)        # (+ 0: no -0.0, whose place in a maximum is nobody's contract)


def _integer_map(case, layer):
    N, Hl, Wl, C = map_shape(case, layer)
    P = case[2]
    rng = np.random.default_rng(_seed(case, 1000 + layer))
    y = rng.choice(_VALUES, size=(N, Hl, Wl, C), p=_WEIGHTS).astype(np.float32)
    _share_pixels(y, P, rng)
    for pair, spot in forced_spots(case, layer).items():
        i0, i1 = pair, P + pair
        r, c = spot["in0_zero"]
        y[i0, r, c] = _non_positive(y[i0, r, c])
        y[i1, r, c, pair % C] = 2
        r, c = spot["in1_zero"]
        y[i1, r, c] = _non_positive(y[i1, r, c])
        y[i0, r, c, (pair + 1) % C] = 3
        r, c = spot["both_zero"]
        y[i0, r, c], y[i1, r, c] = _non_positive(y[i0, r, c]), _non_positive(y[i1, r, c])
        r, c = spot["equal"]
        y[i0, r, c, (pair + 2) % C] = 1
        y[i1, r, c] = y[i0, r, c]
        r, c = spot["negative_window"]
        ch = (7 * pair + 5) % C
        y[i0, r:r + 2, c:c + 2, ch] = [[-1, -3], [-2, -1]]
        y[i1, r:r + 2, c:c + 2, ch] = [[-2, -2], [-3, -1]]
    return y


def _float_map(case, layer):
    rng = np.random.default_rng(_seed(case, 2000 + layer))
    y = (rng.standard_normal(map_shape(case, layer), dtype=np.float32) - np.float32(0.3)).astype(np.float32)
    _share_pixels(y, case[2], rng)
    while True:                       # no exact zero: -0.0 against +0.0 must not decide a bit comparison of the pool
        zero = y == 0
        if not zero.any():
            return y
        y[zero] = rng.standard_normal(int(zero.sum()), dtype=np.float32) - np.float32(0.3)


@functools.lru_cache(maxsize=2)
def integer_maps(case_index):
    """{layer: (2P, Hl, Wl, C) float32} of CASES[case_index], values in {-3 .. 3}: every product and every fp32 sum of the tap is exact
    (a sum of squares is at most 9 x 512).  Shared and cached: read-only."""
    case = CASES[case_index]
    out = {l: _integer_map(case, l) for l in sorted(case[3])}
    for y in out.values():
        y.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def float_maps(case_index):
    """{layer: (2P, Hl, Wl, C) float32} of CASES[case_index]: standard normal minus 0.3, no exact zero.  Shared and cached: read-only."""
    case = CASES[case_index]
    out = {l: _float_map(case, l) for l in sorted(case[3])}
    for y in out.values():
        y.setflags(write=False)
    return out


# ---- the fp64 reference
def norms64(y):
    """(N, Hl, Wl, C) -> (N, Hl, Wl) float64: the Euclidean norm of relu(y) per pixel"""
    r = np.maximum(y, 0).astype(np.float64)
    return np.sqrt(np.einsum("nhwc,nhwc->nhw", r, r))


def tap64(y, P):
    """y (2P, Hl, Wl, C), image i in0 of pair i and image P + i its in1 -> (P,) float64: the mean over pixels of
    dot(r0, r1) / ((|r0| + 1e-10)(|r1| + 1e-10)), r = max(y, 0)"""
    assert y.shape[0] == 2 * P
    out = np.empty(P)
    for i in range(P):
        r0, r1 = np.maximum(y[i], 0).astype(np.float64), np.maximum(y[P + i], 0).astype(np.float64)
        dot = np.einsum("hwc,hwc->hw", r0, r1)
        n0, n1 = np.sqrt(np.einsum("hwc,hwc->hw", r0, r0)), np.sqrt(np.einsum("hwc,hwc->hw", r1, r1))
        out[i] = (dot / ((n0 + 1e-10) * (n1 + 1e-10))).mean()
    return out


def scores64(maps, P):
    """maps {layer: y} (a layer that is not there was not tapped: its workspace block is zero, its score 1) ->
    (layers (P, 5), total (P,)) float64: 1 - mean per layer, and the sum of the five"""
    layers = np.ones((P, LAYERS))
    for l, y in maps.items():
        layers[:, l] = 1.0 - tap64(y, P)
    return layers, layers.sum(1)


def pool(y, relu_first=False):
    """(N, Hl, Wl, C) -> (N, Hl / 2, Wl / 2, C): the 2 x 2 stride-2 maximum of the raw map (relu_first: of its ReLU, which is NOT what
    the tap writes)"""
    if relu_first:
        y = np.maximum(y, 0)
    N, Hl, Wl, C = y.shape
    return y.reshape(N, Hl // 2, 2, Wl // 2, 2, C).max((2, 4))


def rounding_bound(C):
    """The worst case of the kernel's own summation of a layer's score against fp64, float_maps: (2 d + 1) 2^-24.  Every sum (dot,
    |r0|^2, |r1|^2) is one of non-negative terms: a lane adds 4 C / 64 products one after the other, each product and each addition
    rounded once, and the butterfly adds four more levels: d = 4 C / 64 + 5 roundings on the longest path, each of relative size
    2^-24 at most, so each sum is within d 2^-24 of itself, relatively.  A cosine dot / (|r0| |r1|) is at most 1 and carries d 2^-24
    from dot and d / 2 2^-24 from each square root: 2 d 2^-24; the fp64 steps behind add 1e-13, and the score's rounding to fp32
    the last 2^-24 (an ulp of [0.5, 1])."""
    d = 4 * C // 64 + 5
    return (2 * d + 1) * 2.0 ** -24


# ---- the finish alone
def finish_workspace(P, H, W, seed=0):
    """A workspace by the documented layout, [layer][pair][tile] doubles: different multiples of 2^-12 below 1, so that any order of
    addition is exact -> float64 (P * sum tiles,)"""
    n = workspace_bytes(P, H, W) // 8
    assert n < 4096
    return (np.random.default_rng([seed, P, H, W]).permutation(4095)[:n] + 1) * 2.0 ** -12


def finish64(ws, P, H, W):
    """-> (layers (P, 5) float32, total (P,) float32) of a workspace: per layer 1 - sum / pixels, the five added in the layers' order"""
    layers, total = np.empty((P, LAYERS), np.float32), np.empty(P, np.float32)
    for pair in range(P):
        tot = 0.0
        for l in range(LAYERS):
            tiles, o = tiles_of(H, W, l), layer_offset(P, H, W, l)
            score = 1.0 - ws[o + pair * tiles:o + (pair + 1) * tiles].sum() / float((H >> l) * (W >> l))
            layers[pair, l] = np.float32(score)
            tot += score
        total[pair] = np.float32(tot)
    return layers, total
