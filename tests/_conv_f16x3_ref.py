"""Shared by the tests of csrc/conv_f16x3.hip (test_conv_f16x3_walk_gpu.py, test_f16x3_range_gpu.py, test_f16x3_guard_gpu.py, their CPU
companions and _conv_f16x3_wgs_worker.py): a pure-Python mirror of the kernel's launch arithmetic, the host split, the fp64 reference
`T` of what the kernel computes, and the per-element error measure.  No test in here.

The mirror restates ps_conv3x3_f16x3_ex_nhwc's grid and the kernel's item_at / live_of line by line, so that a test can ASSERT that
the launch it is about to make walks several items, changes frame inside a walk, kills and revives a wave -- on the card at hand, with the
PS_CONV_WGS in force -- instead of hoping so.

The measure.  With xa the activated input in fp32 exactly as the kernel forms it (x * scale, then - shift, two roundings: the library is
built with -ffp-contract=off, the kernel compiles to v_mul_f32 / v_sub_f32 (v_pk_mul_f32 / v_pk_add_f32 with a negated operand), no
FMA; torch's eager mul and sub are two kernels, so the host form is bit-equal), split as the kernel splits (hi = fp16(v), lo =
fp16(v - hi)),
    T   = conv64(xh, wh) + conv64(xh, wl) + conv64(xl, wh) (+ bias + res)          what the kernel computes, up to fp32 summation order
    S   = conv64(|xh|, |wh|)                                                         per element: the size of what was summed
    y32 = torch's fp32 convolution of [xh, xh, xl] x [wh, wl, wh] (+ bias + res)     exact fp32 products (11 x 11 bits): another order
    r16 = max |y - T| / S,   r32 = max |y32 - T| / S,   assert r16 <= K * r32, K = 10   (the margin tests/test_block_routes_gpu.py and
                                                                                          the older e16 < 10 * e32 give "another order")
and, end to end, max |y - conv64(xa, w)| / max |conv64(xa, w)| < 3e-6 as tests/test_networks_gpu.py holds it.
"""
import os
from collections import namedtuple

import torch

TH = TW = 16      # output pixels per item
COT = 128         # output channels per item
K16 = 10.0        # r16 <= K16 * r32
END_TO_END = 3e-6

Launch = namedtuple("Launch", "grid J nblocks ncb tiles_x tiles_per_frame live")
Item = namedtuple("Item", "L b ty tx cb")


def wgs_in_force():
    """PS_CONV_WGS as the library reads it (atoi; unset: -1 = one workgroup per compute unit)"""
    e = os.environ.get("PS_CONV_WGS")
    if e is None:
        return -1
    try:
        return int(e.strip() or 0)
    except ValueError:
        return 0


def launch(B, H, W, Co, co_live=0, cus=256, wgs=-1):
    """The launch ps_conv3x3_f16x3_ex_nhwc makes of (B, H, W, *) -> Co channels on a device of `cus` compute units"""
    tiles_x = W // TW
    tpf = (H // TH) * tiles_x
    ncb = (Co + COT - 1) // COT
    nb = B * tpf * ncb
    per_cu = cus // 8 * 8 if cus >= 8 else 8
    cap = (nb + 7) // 8 * 8
    want = per_cu if wgs < 0 else cap if wgs == 0 else (wgs + 7) // 8 * 8
    grid = min(want, cap)
    return Launch(grid, grid >> 3, nb, ncb, tiles_x, tpf, co_live if 0 < co_live < Co else Co)


def walk(ln, block):
    """The items workgroup `block` of the launch walks, in order (the kernel's item_at)"""
    xcd, j0 = block & 7, block >> 3
    lo, hi = (ln.nblocks * xcd) >> 3, (ln.nblocks * (xcd + 1)) >> 3
    out = []
    L = lo + j0
    while L < hi:
        cb, tile = L % ln.ncb, L // ln.ncb
        b, tf = tile // ln.tiles_per_frame, tile % ln.tiles_per_frame
        out.append(Item(L, b, (tf // ln.tiles_x) * TH, (tf % ln.tiles_x) * TW, cb))
        L += ln.J
    return out


def walks(ln):
    return [walk(ln, blk) for blk in range(ln.grid)]


def live_of(ln, item, chh):
    """Does wave half chh (0: waves 0-3, 1: waves 4-7) of the workgroup multiply on this item?"""
    return item.cb * COT + chh * 64 < ln.live


def properties(ln):
    """What the cases assert before they launch.  Transitions are counted between consecutive items of one workgroup."""
    p = dict(items=0, longest=0, dead_to_live=[0, 0], live_to_dead=[0, 0], frame_changes=0, row_changes=0, cb_changes=0, pairs=0,
             all_dead_items=0)
    seen = set()
    for w in walks(ln):
        p["items"] += len(w)
        p["longest"] = max(p["longest"], len(w))
        seen.update(it.L for it in w)
        p["all_dead_items"] += sum(not live_of(ln, it, 0) for it in w)
        for a, b in zip(w, w[1:]):
            p["pairs"] += 1
            p["frame_changes"] += a.b != b.b
            p["row_changes"] += a.b == b.b and a.ty != b.ty
            p["cb_changes"] += a.cb != b.cb
            for chh in (0, 1):
                la, lb = live_of(ln, a, chh), live_of(ln, b, chh)
                p["dead_to_live"][chh] += (not la) and lb
                p["live_to_dead"][chh] += la and not lb
    p["covered"] = seen == set(range(ln.nblocks)) and p["items"] == ln.nblocks     # every item walked exactly once
    return p


def device_launch(B, H, W, Co, co_live=0):
    """The launch this process makes on cuda:0: its compute units, the PS_CONV_WGS in force"""
    return launch(B, H, W, Co, co_live, cus=torch.cuda.get_device_properties(0).multi_processor_count, wgs=wgs_in_force())


def smallest_batch(want, H, W, Co, co_live=0, limit=400):
    """-> (B, properties): the smallest batch whose launch on this card has the property `want(properties)`; AssertionError if none"""
    for B in range(1, limit):
        p = properties(device_launch(B, H, W, Co, co_live))
        assert p["covered"]
        if want(p):
            return B, p
    raise AssertionError(f"no batch below {limit} gives the launch its property on this card")


def nth_item_frames(ln, n):
    """Frames b that are the n-th (0-based) item of some workgroup"""
    return sorted({w[n].b for w in walks(ln) if len(w) > n})


# ---- the host split and the reference ---------------------------------------------------------------------------------------------------
def split(v):
    """v (fp32) -> (hi, lo) as fp32 tensors: hi = fp16(v), lo = fp16(v - hi), round to nearest even, fp16 subnormals kept -- the
    kernel's stash() and k_pack"""
    hi = v.to(torch.float16).to(torch.float32)
    lo = (v - hi).to(torch.float16).to(torch.float32)
    return hi, lo


def activated(x, sc=None, sh=None):
    """max(x * sc - sh, 0) in fp32, one multiply and one subtract (no FMA), NaN kept; x (B, C, H, W), sc / sh (B, C)"""
    if sc is None:
        return x
    B, C = sc.shape
    v = x * sc.view(B, C, 1, 1)
    v = v - sh.view(B, C, 1, 1)
    return torch.relu(v)


def s2d(x):
    """(B, C, 2 H, 2 W) -> (B, 4 C, H, W), channel (sy, sx, c): the form in_s2d reads in place"""
    B, C, H2, W2 = x.shape
    return x.view(B, C, H2 // 2, 2, W2 // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 4 * C, H2 // 2, W2 // 2)


def d2s(y):
    """(B, 4 C, H, W), channel (py, px, c) -> (B, C, 2 H, 2 W): what out_d2s stores"""
    B, C4, H, W = y.shape
    C = C4 // 4
    return y.view(B, 2, 2, C, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, C, 2 * H, 2 * W)


def conv64(x, w):
    return torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)


Reference = namedtuple("Reference", "T S y32 ref xa")


def reference(xa, w, bias=None, res=None):
    """xa (B, Ci, H, W) the activated input, w (Co, Ci, 3, 3); bias (Co), res (B, Co, H, W) or None -> Reference, all (B, Co, H, W)"""
    xh, xl = split(xa)
    wh, wl = split(w)
    # T in one pass: conv(xh, wh + wl) + conv(xl, wh); wh + wl is exact in fp64
    T = conv64(torch.cat([xh, xl], 1), torch.cat([wh.double() + wl.double(), wh.double()], 1))
    S = conv64(xh.abs(), wh.abs())
    y32 = torch.nn.functional.conv2d(torch.cat([xh, xh, xl], 1), torch.cat([wh, wl, wh], 1), None, 1, 1)
    ref = conv64(xa, w)
    for extra in (None if bias is None else bias.view(1, -1, 1, 1), res):
        if extra is not None:
            T = T + extra.double()
            ref = ref + extra.double()
            y32 = y32 + extra
    return Reference(T, S, y32, ref, xa)


def measure(y, r):
    """-> dict(r16, r32, ratio, e2e).  Elements with S = 0 (an all-zero window, all-zero weights) must be exactly the fp32 value of
    bias + res and are left out of the ratios."""
    yd = y.double()
    pos = r.S > 0
    assert torch.equal(y[~pos], r.T[~pos].float()), "an output with nothing to sum is not exactly bias + res"
    S = torch.where(pos, r.S, torch.ones_like(r.S))
    r16 = ((yd - r.T).abs() / S)[pos].max().item()
    r32 = ((r.y32.double() - r.T).abs() / S)[pos].max().item()
    e2e = (yd - r.ref).abs().max().item() / r.ref.abs().max().item()
    return dict(r16=r16, r32=r32, ratio=r16 / r32 if r32 > 0 else float("inf") if r16 > 0 else 0.0, e2e=e2e)


def hold(y, r, what, live=0, pad=None, end_to_end=True):
    """The assertions of every case: no NaN left of the prefill, channels from `live` on exactly `pad` (bias + res in fp32),
    r16 <= K16 * r32, the end-to-end bound (end_to_end=False: reported only -- inputs below 2^-3, where the split itself keeps 2^-25
    absolute and not 22 bits).  Prints the figures before it asserts."""
    assert y.shape == r.T.shape, (what, y.shape, r.T.shape)
    assert not torch.isnan(y).any(), f"{what}: outputs never written"
    if live:
        assert torch.equal(y[:, live:], pad.expand_as(y)[:, live:]), f"{what}: padding channels are not exactly bias + res"
    m = measure(y, r)
    print(f"{what}: r16 {m['r16']:.3e} r32 {m['r32']:.3e} r16/r32 {m['ratio']:.2f} end-to-end {m['e2e']:.2e}")
    assert m["r16"] <= K16 * m["r32"], (what, m)
    assert not end_to_end or m["e2e"] < END_TO_END, (what, m)
    return m


# ---- the kernel through the C ABI ---------------------------------------------------------------------------------------------------------
def pack(w):
    """(Co, Ci, 3, 3) on the device -> packed bytes"""
    from pixelsynth_amd import _lib
    L = _lib.lib()
    Co, Ci = w.shape[:2]
    wl = w.permute(0, 2, 3, 1).contiguous()
    packed = torch.empty(L.ps_conv3x3_f16x3_packed_bytes(Co, Ci), dtype=torch.uint8, device=w.device)
    _lib.check(L.ps_conv3x3_f16x3_pack(wl.data_ptr(), Co, Ci, packed.data_ptr(), torch.cuda.current_stream().cuda_stream), "pack")
    return packed


def run(x, packed, Co, sc=None, sh=None, bias=None, res=None, co_live=0, in_s2d=False, out_d2s=False):
    """ps_conv3x3_f16x3_ex_nhwc on x (B, C, H, W) NCHW values (for in_s2d: the real (B, C, 2 H, 2 W) tensor; Ci = 4 C), res (B, Co, H, W)
    NCHW values; y is filled with NaN first.  -> (y as an NCHW view -- (B, Co / 4, 2 H, 2 W) for out_d2s --, flag)"""
    from pixelsynth_amd import _lib
    L = _lib.lib()
    B, C, H, W = x.shape
    Ci = C
    if in_s2d:
        Ci, H, W = 4 * C, H // 2, W // 2
    xl = x.permute(0, 2, 3, 1).contiguous()
    rl = None
    if res is not None:      # 64 floats of NaN behind res: a load past the last pixel's channels (what ok1 guards for Co = 64) stays inside
        buf = torch.full((res.numel() + 64,), float("nan"), device=x.device)          # the allocation, and shows if it is ever stored
        rl = buf[:res.numel()].view(B, H, W, Co)
        rl.copy_(res.permute(0, 2, 3, 1))
    y = torch.full((B, 2 * H, 2 * W, Co // 4) if out_d2s else (B, H, W, Co), float("nan"), device=x.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(L.ps_conv3x3_f16x3_ex_nhwc(xl.data_ptr(), p(sc), p(sh), packed.data_ptr(), p(bias), p(rl), B, H, W, Ci, Co, co_live, int(in_s2d),
                                          int(out_d2s), y.data_ptr(), flag.data_ptr(), torch.cuda.current_stream().cuda_stream), "conv")
    return y.permute(0, 3, 1, 2), flag


def with_extras(r, bias=None, res=None):
    """A Reference of the plain convolution with bias (Co) and / or res (B, Co, H, W) added the way the kernel adds them"""
    T, y32, ref = r.T, r.y32, r.ref
    for extra in (None if bias is None else bias.view(1, -1, 1, 1), res):
        if extra is not None:
            T, ref, y32 = T + extra.double(), ref + extra.double(), y32 + extra
    return Reference(T, r.S, y32, ref, r.xa)


# ---- the small set tests/_conv_f16x3_wgs_worker.py runs under another PS_CONV_WGS (and its parent under the default grid) ------------------
WGS_B, WGS_HW, WGS_CI = 4, 32, 64


def wgs_cases():
    """Co in {64, 192, 320} x co_live in {0, 100} (Co = 64 takes no hint beyond Co: 40 there), Ci = 64, fused; one s2d, one d2s"""
    cases = [dict(kind="plain", Co=Co, live=min(live, 40) if Co == 64 else live) for Co in (64, 192, 320) for live in (0, 100)]
    return cases + [dict(kind="s2d", Co=128, live=0), dict(kind="d2s", Co=256, live=0)]


def wgs_case_name(c):
    return f"{c['kind']}_{c['Co']}_{c['live']}"


def wgs_case_inputs(c, dev):
    """Deterministic inputs of a case, on `dev`: dict(x, w (Co, Ci, 3, 3) as the kernel is fed, sc, sh, bias, kw)"""
    from pixelsynth_amd.vqvae2.vqvae import convt_weight, s2d_weight
    B, H, Ci, Co = WGS_B, WGS_HW, WGS_CI, c["Co"]
    g = torch.Generator().manual_seed(1000 + Co + c["live"] + len(c["kind"]))
    kw = dict(co_live=c["live"], in_s2d=c["kind"] == "s2d", out_d2s=c["kind"] == "d2s")
    if c["kind"] == "s2d":                                  # real input (B, 32, 2 H, 2 W), read as (B, 128, H, W)
        x = torch.randn(B, 32, 2 * H, 2 * H, generator=g) * 1.5
        w = s2d_weight(torch.randn(Co, 32, 4, 4, generator=g) / (4 * 32 ** 0.5))
        Ci = 128
    elif c["kind"] == "d2s":                                # (B, 64, H, W) -> (B, 64, 2 H, 2 W)
        x = torch.randn(B, Ci, H, H, generator=g) * 1.5
        w = convt_weight(torch.randn(Ci, Co // 4, 4, 4, generator=g) / (2 * Ci ** 0.5))
    else:
        x = torch.randn(B, Ci, H, H, generator=g) * 1.5
        w = torch.randn(Co, Ci, 3, 3, generator=g) / (3 * Ci ** 0.5)
        if c["live"]:
            w[c["live"]:] = 0
    sc, sh = torch.rand(B, Ci, generator=g) + 0.5, torch.randn(B, Ci, generator=g) * 0.3
    bias = torch.randn(Co // 4 if c["kind"] == "d2s" else Co, generator=g)
    if c["kind"] == "d2s":
        bias = bias.repeat(4)
    return dict(x=x.to(dev), w=w.to(dev).contiguous(), sc=sc.to(dev), sh=sh.to(dev), bias=bias.to(dev), kw=kw, Co=Co)


def wgs_case_run(inp):
    """-> (y, flag) of the case on the current PS_CONV_WGS"""
    return run(inp["x"], pack(inp["w"]), inp["Co"], inp["sc"], inp["sh"], inp["bias"], None, **inp["kw"])
