"""CPU: the pure-Python mirror of csrc/conv_f16x3.hip's launch arithmetic (tests/_conv_f16x3_ref.py) on launches worked out by hand
from the kernel's item_at and the wrapper's grid.  The GPU tests assert their launch properties on this mirror before they launch, so
its own arithmetic is pinned here, without a GPU."""
import _conv_f16x3_ref as M


def test_one_tile_lands_on_the_last_xcd():
    """B = 1, 16 x 16, Co = 128: one item.  grid = min(256, 8) = 8, J = 1; lo_x = (1 * x) >> 3 = 0 for every x, hi_x = (x + 1) >> 3 = 1
    for x = 7 alone: block 7 walks item 0, the other seven return at once."""
    ln = M.launch(1, 16, 16, 128, cus=256)
    assert ln == M.Launch(grid=8, J=1, nblocks=1, ncb=1, tiles_x=1, tiles_per_frame=1, live=128)
    assert [len(w) for w in M.walks(ln)] == [0, 0, 0, 0, 0, 0, 0, 1]
    assert M.walk(ln, 7) == [M.Item(L=0, b=0, ty=0, tx=0, cb=0)]


def test_three_channel_blocks_under_an_even_stride():
    """B = 11, 64 x 64, Co = 320 on 256 compute units: 11 * 16 tiles * 3 blocks = 528 items, grid 256, J = 32, 66 items per XCD, so
    workgroups j0 = 0, 1 of each XCD walk 3 items and the others 2.  The stride 32 = 2 (mod 3): cb changes at every step.
    Workgroup 0: L = 0, 32, 64 -> (tile 0, cb 0), (tile 10, cb 2) = row 2, column 2 of frame 0, (tile 21, cb 1) = tile 5 of frame 1.
    Workgroup 255 (XCD 7, j0 = 31): lo = 528 * 7 >> 3 = 462, L = 493, 525 -> (tile 164 = frame 10 tile 4, cb 1), (tile 175 = frame 10
    tile 15, cb 0)."""
    ln = M.launch(11, 64, 64, 320, cus=256)
    assert (ln.grid, ln.J, ln.nblocks, ln.ncb, ln.tiles_per_frame) == (256, 32, 528, 3, 16)
    assert M.walk(ln, 0) == [M.Item(0, 0, 0, 0, 0), M.Item(32, 0, 32, 32, 2), M.Item(64, 1, 16, 16, 1)]
    assert M.walk(ln, 255) == [M.Item(493, 10, 16, 0, 1), M.Item(525, 10, 48, 48, 0)]
    assert sorted(len(w) for w in M.walks(ln)) == [2] * 240 + [3] * 16
    p = M.properties(ln)
    assert p["covered"] and p["items"] == 528 and p["longest"] == 3 and p["cb_changes"] == p["pairs"] == 272
    # block 2 = channels 256 .. 383 of which 320 .. 383 are padding: wave half 1 is dead there and nowhere else
    assert p["dead_to_live"] == [0, 88] and p["live_to_dead"] == [0, 96] and p["all_dead_items"] == 0
    # Co = 384 with 200 live channels: block 1's upper half and all of block 2 are dead
    ln = M.launch(11, 64, 64, 384, co_live=200, cus=256)
    p = M.properties(ln)
    assert ln.live == 200 and p["dead_to_live"] == [88, 88] and p["live_to_dead"] == [96, 96] and p["all_dead_items"] == 528 // 3


def test_one_workgroup_per_xcd_walks_its_whole_run():
    """PS_CONV_WGS = 8, B = 4, 32 x 32, Co = 320: 48 items, grid 8, J = 1: XCD x walks L = 6 x .. 6 x + 5, cb = 0, 1, 2, 0, 1, 2 over two
    tiles; XCD 1: tiles 2, 3 of frame 0 (row 1), XCD 2: tiles 0, 1 of frame 1."""
    ln = M.launch(4, 32, 32, 320, cus=256, wgs=8)
    assert (ln.grid, ln.J, ln.nblocks) == (8, 1, 48)
    assert M.walk(ln, 1) == [M.Item(6, 0, 16, 0, 0), M.Item(7, 0, 16, 0, 1), M.Item(8, 0, 16, 0, 2),
                             M.Item(9, 0, 16, 16, 0), M.Item(10, 0, 16, 16, 1), M.Item(11, 0, 16, 16, 2)]
    assert [it.b for it in M.walk(ln, 2)] == [1] * 6 and [it.cb for it in M.walk(ln, 2)] == [0, 1, 2, 0, 1, 2]
    w = M.walk(ln, 1)
    assert [M.live_of(ln, it, 1) for it in w] == [True, True, False, True, True, False]
    assert all(M.live_of(ln, it, 0) for it in w)
    p = M.properties(ln)
    assert p["longest"] == 6 and p["dead_to_live"] == [0, 8] and p["live_to_dead"] == [0, 16] and p["covered"]
    # 5 and 9 workgroups asked for: rounded up to the eight XCDs
    assert M.launch(4, 32, 32, 320, cus=256, wgs=5).grid == 8 and M.launch(4, 32, 32, 320, cus=256, wgs=9).grid == 16


def test_one_item_per_workgroup_and_counts_the_xcds_do_not_divide():
    """PS_CONV_WGS = 0, B = 5, 32 x 32, Co = 64: 20 items, grid 24, J = 3.  lo_x = 20 x >> 3 = 0, 2, 5, 7, 10, 12, 15, 17, 20: the XCDs
    take 2, 3, 2, 3, ... items; workgroup j0 = 2 of an XCD with two items has none."""
    ln = M.launch(5, 32, 32, 64, cus=256, wgs=0)
    assert (ln.grid, ln.J, ln.nblocks, ln.live) == (24, 3, 20, 64)
    counts = [len(M.walk(ln, blk)) for blk in range(24)]
    assert max(counts) == 1 and sum(counts) == 20
    assert [blk for blk in range(24) if counts[blk] == 0] == [16, 18, 20, 22]      # j0 = 2 (blocks 16 .. 23) of XCDs 0, 2, 4, 6
    assert M.walk(ln, 9) == [M.Item(L=3, b=0, ty=16, tx=16, cb=0)]                 # XCD 1, j0 = 1: lo = 2
    assert M.properties(ln)["covered"]
    # 64 output channels: the upper half of the only block is padding for every item
    assert not M.live_of(ln, M.walk(ln, 9)[0], 1) and M.live_of(ln, M.walk(ln, 9)[0], 0)


def test_compute_unit_counts_and_the_live_hint():
    assert M.launch(70, 32, 32, 128, cus=20).grid == 16         # a multiple of eight, rounded down
    assert M.launch(70, 32, 32, 128, cus=4).grid == 8           # at least eight
    assert M.launch(70, 32, 32, 128, cus=304).grid == 280 and M.launch(70, 32, 32, 128, cus=304).J == 35
    assert M.launch(1, 16, 16, 256, co_live=0).live == 256 and M.launch(1, 16, 16, 256, co_live=256).live == 256
    assert M.launch(1, 16, 16, 256, co_live=1).live == 1
    # B = 70 at 32 x 32 with one or two channel blocks under J = 32 (the older direct test): several items, but no wave ever changes state
    for Co in (64, 128, 256):
        p = M.properties(M.launch(70, 32, 32, Co, cus=256))
        assert p["longest"] >= 2 and p["dead_to_live"] == [0, 0] and p["live_to_dead"] == [0, 0]
    ln = M.launch(40, 64, 64, 128, cus=256)
    assert M.nth_item_frames(ln, 2) == sorted({M.walk(ln, blk)[2].b for blk in range(256) if len(M.walk(ln, blk)) > 2})
    assert M.properties(ln)["frame_changes"] == M.properties(ln)["pairs"] == 384    # stride 32 tiles = two frames at every step
