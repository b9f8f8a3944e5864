"""Cases the FID convolution's edge tests share (tests/test_fid_edges_cpu.py on the table alone, tests/test_fid_conv_edges_gpu.py on the
kernel): shapes off the network's, integer-valued operands whose convolution is exact in any summation order, and the fp64 reference.
Plain numpy / torch on the CPU; nothing here touches a device.

k_fid_conv (csrc/fid.hip): K = KH KW Ci is walked in groups of 4 channels of one tap (C4 = Ci / 4 groups a tap), 4 groups a chunk, 4
chunks (64 values of K) a stage, S stages; a middle sum is flushed after every fourth stage and after the last.  A workgroup owns
T = ps_fid_conv_co_tile(Co) output channels (64: <MT 4, NT 2>, 128 pixels; 32: <MT 2, NT 4>, 256 pixels); a lane stores 4 channels
at once where they all exist and one by one in the last quad of a Co that is no multiple of 4."""
import numpy as np
import torch
import torch.nn.functional as F

# (KH, KW, stride, ph, pw, Ci, ldx, Co, N, H, W); H, W <= 20, N <= 3, Ci <= 20, Co <= 100
HAND = [
    # Co and the pixel counts N Ho Wo (in brackets), K below 16
    (1, 1, 1, 0, 0, 4, 4, 1, 1, 3, 5),             # K = 4; Co = 1 [15]
    (1, 1, 1, 0, 0, 8, 8, 3, 1, 4, 4),             # K = 8 in two groups [16]
    (1, 2, 1, 0, 0, 4, 8, 5, 1, 1, 18),            # K = 8 in two taps, ldx = Ci + 4 [17]
    (1, 2, 1, 0, 1, 12, 12, 31, 2, 5, 6),          # C4 = 3 [70]
    (2, 2, 1, 1, 1, 8, 20, 32, 1, 10, 11),         # C4 = 2, ldx = Ci + 12 [132]
    (2, 2, 2, 0, 0, 16, 16, 33, 2, 8, 16),         # K = 64: one full stage [64]
    (3, 3, 1, 1, 1, 4, 4, 36, 2, 7, 9),            # T = 64 just under its 128 pixels [126]; a quad ends the third tile
    (3, 3, 2, 1, 1, 8, 8, 63, 2, 16, 16),          # T = 64 at 128 pixels; stride 2 p(1,1), even H and W
    (3, 3, 2, 1, 1, 12, 12, 65, 2, 9, 19),         # stride 2 p(1,1), odd H and W [100]; T = 32, the third block holds one channel
    (4, 4, 1, 3, 3, 16, 16, 64, 1, 7, 10),         # T = 64 over 128 pixels [130]; K = 256, S = 4; padding KH - 1
    (5, 5, 2, 2, 2, 12, 12, 70, 1, 15, 20),        # stride 2 p(2,2) [80]; K = 300, S = 5; Co = 70: a quad and a tail of 2 in block 3
    (5, 5, 1, 2, 2, 4, 16, 96, 1, 16, 16),         # T = 32 at its 256 pixels; three full blocks
    (3, 3, 1, 1, 1, 8, 8, 96, 3, 5, 17),           # T = 32 just under 256 [255]
    (7, 7, 2, 3, 3, 12, 12, 100, 3, 17, 20),       # stride 2 p(3,3) [270]: T = 64, three pixel tiles; K = 588, S = 10; two blocks
    (3, 3, 1, 2, 2, 8, 8, 70, 1, 11, 18),          # T = 32 over 256 [13 x 20 = 260]: a second tile of 4 pixels
    (7, 7, 1, 3, 3, 20, 20, 5, 1, 4, 4),           # 7 x 7 p(3,3) on a 4 x 4 map; K = 980, S = 16 [16]
    # small maps
    (3, 3, 1, 1, 1, 16, 16, 33, 1, 1, 1),          # H = W = 1 [1]
    (1, 7, 1, 0, 3, 8, 8, 31, 3, 5, 2),            # W = 2 under 1 x 7 p(0,3) [30]
    (7, 1, 1, 3, 0, 20, 24, 36, 1, 1, 17),         # H + 2 ph == KH: one output row [17]
    (2, 7, 1, 1, 6, 4, 4, 3, 1, 3, 3),             # padding KH - 1 and KW - 1 [36]
    (7, 2, 2, 3, 1, 12, 12, 70, 1, 11, 12),        # [42]
    # stride 2 with padding, the other parities and the asymmetric ones
    (3, 3, 2, 2, 2, 8, 8, 32, 1, 12, 13),          # p(2,2), even H, odd W [56]
    (4, 4, 2, 3, 3, 20, 20, 1, 2, 10, 7),          # p(3,3), even H, odd W [70]; K = 320, S = 5
    (7, 7, 2, 3, 3, 4, 4, 36, 1, 14, 9),           # p(3,3) [35]; K = 196, S = 4
    (3, 3, 2, 0, 2, 4, 4, 33, 1, 9, 8),            # p(0,2) on a square kernel, odd H, even W [20]
    (5, 5, 2, 0, 2, 8, 12, 64, 2, 10, 11),         # p(0,2), even H, odd W [36]
    (3, 3, 2, 2, 0, 20, 20, 63, 1, 8, 9),          # p(2,0), even H, odd W [20]
    (7, 7, 2, 2, 0, 4, 4, 100, 1, 13, 14),         # p(2,0), odd H, even W [24]
    (5, 5, 2, 2, 2, 16, 28, 5, 2, 16, 11),         # 5 x 5 at stride 2, ldx = Ci + 12 [96]
]

KERNELS = [(1, 1), (1, 2), (2, 2), (3, 3), (4, 4), (5, 5), (7, 7), (2, 7), (7, 2), (1, 7), (7, 1)]
CIS = [4, 8, 12, 16, 20]
COS = [1, 3, 5, 31, 32, 33, 36, 63, 64, 65, 70, 96, 100]


def _cross():
    """Every kernel of KERNELS on every Ci of CIS, on a small map: the tap walk at C4 = 1 .. 5 under every kernel; Co, ldx, stride and
    padding cycle through their values."""
    out = []
    for a, (kh, kw) in enumerate(KERNELS):
        for b, ci in enumerate(CIS):
            k = 5 * a + b
            stride = 1 + k % 2
            ph, pw = (k // 2) % kh, (k // 3) % kw
            H, W = max(kh - 2 * ph, 1) + 2 + k % 4, max(kw - 2 * pw, 1) + 3 + k % 5
            out.append((kh, kw, stride, ph, pw, ci, ci + (0, 4, 12)[k % 3], COS[k % len(COS)], 1 + k % 3, H, W))
    return out


CASES = HAND + _cross()

# the rounding cases of the GPU file: K = 256, 320, 1024 and 1040 on a 9 x 9 map (randn operands, the 4 x torch bound)
ROUNDING = [
    (4, 4, 1, 1, 1, 16, 16, 36, 2, 9, 9),          # K = 256: S = 4, the flush on the last stage
    (4, 4, 1, 1, 1, 20, 20, 36, 2, 9, 9),          # K = 320: S = 5
    (2, 2, 1, 1, 1, 256, 256, 36, 2, 9, 9),        # K = 1024: S = 16, four full middle sums
    (2, 2, 1, 1, 1, 260, 260, 36, 2, 9, 9),        # K = 1040: S = 17, a fifth middle sum of one stage, a quarter full
]


def out_shape(case):
    KH, KW, s, ph, pw, _, _, _, _, H, W = case
    return (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1


def pixels(case):
    Ho, Wo = out_shape(case)
    return case[8] * Ho * Wo


def K_of(case):
    return case[0] * case[1] * case[5]


def stages(case):
    return (K_of(case) + 63) // 64


def co_tile(Co):
    """ps_fid_conv_co_tile restated: 32 where that pads Co less than 64 does"""
    return 32 if (Co + 31) // 32 * 32 < (Co + 63) // 64 * 64 else 64


def name(case):
    KH, KW, s, ph, pw, Ci, ldx, Co, N, H, W = case
    return f"{KH}x{KW}s{s}p{ph}{pw}-{Ci}of{ldx}-{Co}-{N}x{H}x{W}"


def integer_operands(index):
    """-> x (N, H, W, Ci), w (Co, Ci, KH, KW), bias (Co) of CASES[index]: integer-valued float32, x and w uniform in {-3 .. 3}, the bias
    in {-8 .. 8}.  |any partial sum| <= 9 K + 8 <= 8828 < 2^24: exact in fp32 in any order."""
    KH, KW, _, _, _, Ci, _, Co, N, H, W = CASES[index]
    rs = np.random.RandomState(1 + index)     # (a base seed under which every case keeps a quarter nonzero)
    x = rs.randint(-3, 4, size=(N, H, W, Ci)).astype(np.float32)
    w = rs.randint(-3, 4, size=(Co, Ci, KH, KW)).astype(np.float32)
    return x, w, rs.randint(-8, 9, size=(Co,)).astype(np.float32)


def randn_operands(case, seed, N=None):
    """-> x (N, H, W, Ci), w (Co, Ci, KH, KW) of variance 2 / K, bias (Co) of a case tuple: float32 normal deviates"""
    KH, KW, _, _, _, Ci, _, Co, n, H, W = case
    rs = np.random.RandomState(seed)
    x = rs.randn(N or n, H, W, Ci).astype(np.float32)
    w = (rs.randn(Co, Ci, KH, KW) * (2.0 / (KH * KW * Ci)) ** 0.5).astype(np.float32)
    return x, w, (rs.randn(Co) * 0.1).astype(np.float32)


def reference(x, w, bias, case):
    """relu(conv2d) of NHWC x in fp64 on the CPU -> (N, Ho, Wo, Co) float64 tensor"""
    _, _, s, ph, pw = case[:5]
    y = F.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double(), torch.from_numpy(bias).double(), s, (ph, pw))
    return torch.relu(y).permute(0, 2, 3, 1).contiguous()


def widen(x, ldx, fill=np.nan):
    """x (N, H, W, Ci) as the leading channels of an (N, H, W, ldx) map whose other channels hold `fill`"""
    out = np.full(x.shape[:3] + (ldx,), fill, dtype=np.float32)
    out[..., :x.shape[3]] = x
    return out


def same_patch_operands(case, seed):
    """The order test's operands: one weight row and one bias for every output channel, and an input of period `stride` in h and w (no
    padding), so that every output pixel reads the same KH x KW x Ci values: all N Ho Wo x Co outputs are one sum.  The sign of the
    weights is chosen so that the sum is positive (the ReLU would make any two negative sums equal).
    -> x, w, bias, the value in fp64"""
    KH, KW, s, ph, pw, Ci, _, Co, N, H, W = case
    assert ph == 0 and pw == 0
    rs = np.random.RandomState(seed)
    base = rs.randn(s, s, Ci).astype(np.float32)
    x = np.ascontiguousarray(np.broadcast_to(np.tile(base, ((H + s - 1) // s, (W + s - 1) // s, 1))[:H, :W], (N, H, W, Ci)))
    row = (rs.randn(Ci, KH, KW) * (2.0 / (KH * KW * Ci)) ** 0.5).astype(np.float32)
    b = np.float32(0.1)
    value = sum(float(row[c, kh, kw]) * float(base[kh % s, kw % s, c]) for c in range(Ci) for kh in range(KH) for kw in range(KW))
    if value + float(b) <= 0:
        row, value = -row, -value
    return x, np.ascontiguousarray(np.broadcast_to(row, (Co,) + row.shape)), np.full(Co, b, np.float32), value + float(b)


# (KH, KW, stride, 0, 0, Ci, Ci, Co, N, H, W) of the order test: both tile widths, two and three Co blocks, a scalar tail (70), two
# pixel tiles with a ragged second one
SAME_PATCH = [
    (3, 3, 2, 0, 0, 12, 12, 100, 3, 20, 20),       # T = 64, 243 pixels: tiles of 128 and 115; blocks of 64 and 36
    (5, 5, 1, 0, 0, 20, 20, 70, 3, 14, 14),        # T = 32, 300 pixels: tiles of 256 and 44; blocks of 32, 32 and 6; K = 500
    (3, 2, 2, 0, 0, 12, 12, 70, 3, 19, 20),        # T = 32, 270 pixels at stride 2
    (5, 5, 1, 0, 0, 20, 20, 100, 3, 14, 14),
]
