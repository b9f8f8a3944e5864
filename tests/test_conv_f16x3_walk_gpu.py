"""GPU: the persistent item walk of csrc/conv_f16x3.hip against fp64.  A workgroup walks several (tile, channel block) items with the
chunk pipeline running across them: the next item's patch (and its frame's scale / shift) is fetched during the current item's last
chunk, the results leave behind the next item's first taps, and a wave whose 64-channel half is padding goes dead and has to read its first
fragments itself when it comes back (`fresh`).  Every case first ASSERTS, on the mirror of the launch arithmetic
(tests/_conv_f16x3_ref.py, fed this card's compute units and the PS_CONV_WGS in force), that its launch has the property it is about
-- the batch is the smallest one for which it does -- and then holds the result to the reference and the measure described there:
per element against T (the three split products in fp64), scaled by S, r16 <= 10 r32; and 3e-6 end to end against conv64(xa, w).

Shapes: 64 x 64 frames (a 4 x 4 tile grid: interior tiles, every border, tile rows inside a frame), the fewest channels that show the
property, and the smallest batch that gives some workgroup three items (on 256 compute units: more than 512 items, 131 000 output pixels).

Every case prints r16, r32, their ratio and the end-to-end error before it asserts (pytest -s); the figures are not recorded here yet.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _conv_f16x3_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_launch, _smallest_batch = M.device_launch, M.smallest_batch


def _draw(seed, B, Ci, H, W, Co, fuse=True, live=0, xs=1.5):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, Ci, H, W, generator=g) * xs).to(DEV)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
    if live:
        w[live:] = 0
    # a scale / shift of its own for every frame, O(1) apart: a neighbour frame's affine moves the result by tenths, not by 1e-6
    sc = (torch.rand(B, Ci, generator=g) + 0.5).to(DEV) if fuse else None
    sh = (torch.randn(B, Ci, generator=g) * 0.3).to(DEV) if fuse else None
    return x, w.to(DEV), sc, sh


_three_items = lambda p: p["longest"] >= 3


@pytest.mark.parametrize("Co,live", [(320, 0), (384, 200)])
def test_waves_die_and_come_back_inside_a_walk(Co, live):
    """Cases 1 and 2.  Co = 320: three channel blocks, the upper half of block 2 is padding; the walk's stride J = grid / 8 is even and
    ncb = 3, so cb changes at EVERY step and the upper wave half dies and revives inside a walk (256 CUs: B = 11, 528 items, 3 per
    workgroup at most, 88 dead -> live and 96 live -> dead transitions).  Co = 384 with co_live = 200: block 1's upper half and ALL of
    block 2 are dead -- whole items without an MFMA, both wave halves revived.  Ci = 64 (two chunks), fused, per-frame affine.
    With and without the skip the results are bit-equal: (384, 200) against co_live = 0; Co = 320 takes no hint (its dead half lies
    beyond Co), so against the same weights zero-padded to 384 channels, where every wave multiplies."""
    H = W = 64
    Ci = 64
    want = lambda p: (p["longest"] >= 3 and p["dead_to_live"][1] > 0 and p["live_to_dead"][1] > 0 and p["frame_changes"] > 0
                      and p["row_changes"] > 0 and (not live or (p["dead_to_live"][0] > 0 and p["all_dead_items"] > 0)))
    B, p = _smallest_batch(want, H, W, Co, live)
    print(f"Co {Co} live {live}: B = {B}, {p}")
    x, w, sc, sh = _draw(Co + live, B, Ci, H, W, Co, live=live)
    bias = torch.randn(Co, generator=torch.Generator().manual_seed(1)).to(DEV)
    r = M.reference(M.activated(x, sc, sh), w, bias)
    y, flag = M.run(x, M.pack(w), Co, sc, sh, bias, co_live=live)
    assert int(flag.item()) == 0
    M.hold(y, r, f"liveness Co {Co} live {live}", live=live, pad=bias.view(1, -1, 1, 1))
    # hint versus no hint over the same walk
    if live:
        assert M.properties(_launch(B, H, W, Co, 0))["dead_to_live"] == [0, 0]
        y_all, _ = M.run(x, M.pack(w), Co, sc, sh, bias, co_live=0)
        assert torch.equal(y, y_all)
    else:
        w384, b384 = torch.cat([w, w.new_zeros(64, Ci, 3, 3)]), torch.cat([bias, bias.new_zeros(64)])
        assert M.properties(_launch(B, H, W, 384, 0))["dead_to_live"] == [0, 0] and _launch(B, H, W, 384).J == _launch(B, H, W, Co).J
        y_all, _ = M.run(x, M.pack(w384), 384, sc, sh, b384)
        assert torch.equal(y, y_all[:, :Co]) and not y_all[:, Co:].any()


@pytest.mark.parametrize("Ci", [32, 64, 96])
def test_the_next_frames_affine_arrives_with_the_next_frames_patch(Ci):
    """Case 3.  Co = 128 (one channel block: consecutive items of a workgroup are different tiles, J tiles apart -- on 256 CUs always two
    frames on), one, two and three chunks per item.  The scale / shift fetched with the next item's first patch must be the NEXT frame's.
    256 CUs: B = 33, 528 items."""
    H = W = 64
    B, p = _smallest_batch(lambda p: p["longest"] >= 3 and p["frame_changes"] > 0, H, W, 128)
    print(f"Ci {Ci}: B = {B}, {p}")
    x, w, sc, sh = _draw(Ci, B, Ci, H, W, 128)
    r = M.reference(M.activated(x, sc, sh), w)
    y, flag = M.run(x, M.pack(w), 128, sc, sh)
    assert int(flag.item()) == 0
    M.hold(y, r, f"fuse across frames Ci {Ci}")


@pytest.mark.parametrize("fuse", [True, False])
def test_space_to_depth_patches_are_aimed_again_for_every_item(fuse):
    """Case 4, in_s2d: x (B, 32, 128, 128) read in place as (B, 128, 64, 64) -- Ci / 4 = 32 is the least the kernel takes, four chunks
    = the four sub-positions -- Co = 128; aim() runs again at every item change.  Against torch's 4 x 4 stride-2 convolution in fp64
    through vqvae.s2d_weight (end to end) and against T of the 3 x 3 form (per element).  256 CUs: B = 33."""
    from pixelsynth_amd.vqvae2.vqvae import s2d_weight
    H = W = 64
    C, Co = 32, 128
    B, p = _smallest_batch(_three_items, H, W, Co)
    print(f"s2d: B = {B}, {p}")
    g = torch.Generator().manual_seed(40 + fuse)
    x = (torch.randn(B, C, 2 * H, 2 * W, generator=g) * 1.5).to(DEV)
    w4 = (torch.randn(Co, C, 4, 4, generator=g) / (4 * C ** 0.5)).to(DEV)
    sc = (torch.rand(B, 4 * C, generator=g) + 0.5).to(DEV) if fuse else None          # per space-to-depth channel (sy, sx, c)
    sh = (torch.randn(B, 4 * C, generator=g) * 0.3).to(DEV) if fuse else None
    bias = torch.randn(Co, generator=g).to(DEV)
    w3 = s2d_weight(w4).contiguous()
    xa = M.activated(M.s2d(x), sc, sh)
    r = M.reference(xa, w3, bias)
    strided = torch.nn.functional.conv2d(M.d2s(xa).double(), w4.double(), bias.double(), 2, 1)     # (d2s undoes s2d: same channel order)
    assert (strided - r.ref).abs().max().item() <= 1e-12 * r.ref.abs().max().item()
    r = r._replace(ref=strided)
    y, flag = M.run(x, M.pack(w3), Co, sc, sh, bias, in_s2d=True)
    assert int(flag.item()) == 0
    M.hold(y, r, f"s2d fuse {fuse}")


@pytest.mark.parametrize("fuse", [True, False])
def test_depth_to_space_stores_follow_the_walk(fuse):
    """Case 4, out_d2s: (B, 32, 64, 64) -> Co = 4 * 64 = 256 (the least: Co / 4 a multiple of 64; two channel blocks = parities
    (0, *) and (1, *)) stored as (B, 64, 128, 128).  Against torch's 4 x 4 stride-2 transposed convolution in fp64 through
    vqvae.convt_weight.  256 CUs: B = 17."""
    from pixelsynth_amd.vqvae2.vqvae import convt_weight
    H = W = 64
    Ci, C = 32, 64
    B, p = _smallest_batch(_three_items, H, W, 4 * C)
    print(f"d2s: B = {B}, {p}")
    g = torch.Generator().manual_seed(50 + fuse)
    x = (torch.randn(B, Ci, H, W, generator=g) * 1.5).to(DEV)
    wt = (torch.randn(Ci, C, 4, 4, generator=g) / (2 * Ci ** 0.5)).to(DEV)
    sc = (torch.rand(B, Ci, generator=g) + 0.5).to(DEV) if fuse else None
    sh = (torch.randn(B, Ci, generator=g) * 0.3).to(DEV) if fuse else None
    bias = torch.randn(C, generator=g).to(DEV)
    w3, b4 = convt_weight(wt).contiguous(), bias.repeat(4).contiguous()
    xa = M.activated(x, sc, sh)
    r = M.reference(xa, w3, b4)
    r = M.Reference(M.d2s(r.T), M.d2s(r.S), M.d2s(r.y32), M.d2s(r.ref), xa)
    transposed = torch.nn.functional.conv_transpose2d(xa.double(), wt.double(), bias.double(), 2, 1)
    assert (transposed - r.ref).abs().max().item() <= 1e-12 * r.ref.abs().max().item()
    r = r._replace(ref=transposed)
    y, flag = M.run(x, M.pack(w3), 4 * C, sc, sh, b4, out_d2s=True)
    assert int(flag.item()) == 0 and y.shape == (B, C, 2 * H, 2 * W)
    M.hold(y, r, f"d2s fuse {fuse}")


@pytest.mark.parametrize("Co", [64, 128, 256])
def test_bias_and_the_other_branch_over_a_walk_against_fp64(Co):
    """Case 5.  bias, res and both; res is loaded behind the previous item's stores (`stored`).  Co = 64: the upper half of the only
    block is padding, ok1 keeps its residual loads and its stores away (the helper puts 64 floats of NaN behind res: a load past the last
    pixel stays inside the allocation and shows if it is ever stored).  Ci = 32, unfused (what a block's second convolution is).  256 CUs: B = 33, 33, 17."""
    H = W = 64
    B, p = _smallest_batch(_three_items, H, W, Co)
    print(f"bias / res Co {Co}: B = {B}, {p}")
    x, w, _, _ = _draw(60 + Co, B, 32, H, W, Co, fuse=False)
    g = torch.Generator().manual_seed(Co)
    bias, res = torch.randn(Co, generator=g).to(DEV), torch.randn(B, Co, H, W, generator=g).to(DEV)
    plain = M.reference(x, w)
    packed = M.pack(w)
    for bb, rr in ((bias, None), (None, res), (bias, res)):
        y, flag = M.run(x, packed, Co, None, None, bb, rr)
        assert int(flag.item()) == 0
        M.hold(y, M.with_extras(plain, bb, rr), f"Co {Co} bias {bb is not None} res {rr is not None}")


@pytest.mark.parametrize("fuse", [True, False])
def test_the_shortest_pipeline(fuse):
    """Case 6.  B = 1, 16 x 16, Ci = 32, Co = 128: one tile, one chunk, one item in the whole launch -- nine taps, the `gg + 2 >= GG`
    and `gg + 3 < GG` tails entered from the very first chunk, no next patch ever fetched."""
    p = M.properties(_launch(1, 16, 16, 128))
    assert p["items"] == 1 and p["longest"] == 1
    x, w, sc, sh = _draw(7 + fuse, 1, 32, 16, 16, 128, fuse=fuse)
    r = M.reference(M.activated(x, sc, sh), w)
    y, flag = M.run(x, M.pack(w), 128, sc, sh)
    assert int(flag.item()) == 0
    M.hold(y, r, f"shortest fuse {fuse}")


def test_another_grid_walks_the_same_items_to_the_same_bits(tmp_path):
    """Case 7.  An item's MFMA order does not depend on who walks it, so the outputs under PS_CONV_WGS = 8 (one workgroup per XCD walks its
    whole run, cb changing at every item for Co > 128) and PS_CONV_WGS = 0 (one item per workgroup, no persistence) must be BIT-equal to
    this process's grid's; any difference is a hand-over fault.  PS_CONV_WGS is read once per process: two fresh children
    (tests/_conv_f16x3_wgs_worker.py), one after the other, each under its own time limit; a child that died ends the test there.
    The set (tests/_conv_f16x3_ref.wgs_cases): B = 4, 32 x 32, Ci = 64, fused, Co in {64, 192, 320} x co_live in {0, 100}, one s2d, one d2s."""
    cus = _cus()
    cases = M.wgs_cases()
    # the properties the children's launches are for
    for c in cases:
        p8 = M.properties(M.launch(M.WGS_B, M.WGS_HW, M.WGS_HW, c["Co"], c["live"], cus=cus, wgs=8))
        p0 = M.properties(M.launch(M.WGS_B, M.WGS_HW, M.WGS_HW, c["Co"], c["live"], cus=cus, wgs=0))
        assert p8["covered"] and p0["covered"] and p0["longest"] == 1 and p8["longest"] == p8["items"] // 8 >= 2
        if c["Co"] > 128:
            assert p8["longest"] >= 4 and p8["cb_changes"] == p8["pairs"]           # cb changes at every step
            if c["kind"] == "plain":
                assert p8["dead_to_live"][1] > 0 and p8["live_to_dead"][1] > 0
                assert not c["live"] or (p8["dead_to_live"][0] > 0 and p8["all_dead_items"] > 0)
    here = {}
    for c in cases:
        inp = M.wgs_case_inputs(c, DEV)
        y, flag = M.wgs_case_run(inp)
        assert int(flag.item()) == 0
        xa = M.activated(M.s2d(inp["x"]) if c["kind"] == "s2d" else inp["x"], inp["sc"], inp["sh"])
        r = M.reference(xa, inp["w"], inp["bias"])
        if c["kind"] == "d2s":
            r = M.Reference(M.d2s(r.T), M.d2s(r.S), M.d2s(r.y32), M.d2s(r.ref), xa)
        M.hold(y, r, f"this grid {M.wgs_case_name(c)}", live=c["live"], pad=inp["bias"].view(1, -1, 1, 1))
        here[M.wgs_case_name(c)] = (y, r, c, inp)
    torch.cuda.synchronize()
    for wgs in ("8", "0"):
        out = str(tmp_path / f"wgs{wgs}.npz")
        child = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conv_f16x3_wgs_worker.py"), out], capture_output=True, text=True,
                               timeout=180, cwd=ROOT, env=dict(os.environ, PS_CONV_WGS=wgs))
        assert child.returncode == 0, f"PS_CONV_WGS={wgs}: exit {child.returncode}\n{child.stderr[-3000:]}"      # (nothing further is started)
        got = np.load(out)
        assert int(got["wgs"]) == int(wgs)
        for name, (y, r, c, inp) in here.items():
            assert int(got[name + "_flag"][0]) == 0
            yc = torch.from_numpy(got[name]).to(DEV)
            M.hold(yc, r, f"PS_CONV_WGS={wgs} {name}", live=c["live"], pad=inp["bias"].view(1, -1, 1, 1))
            assert torch.equal(yc, y), f"PS_CONV_WGS={wgs} {name}: {(yc != y).sum().item()} outputs differ from this process's grid's"
