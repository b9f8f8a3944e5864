"""What the tests of the VGG19 content loss share (test_content_loss_cpu.py, test_content_loss_gpu.py): the loss written out over a state
dict with torch's functions (no module of the package), the backward chain with its decisions frozen, the operator-level formulas and the
bounds.

Bounds.  The loss is Lipschitz in every activation, so the HIP route's values are compared free-running with the same network in fp64:
|L - L64| <= 4 max(|L32 - L64|, 1e-6 L64), L32 torch's fp32 modules (the project's rule: four times the error of the fp32 route that
is being replaced, with a floor of four fp32-sized relative errors for a case where torch's happens to vanish).  The gradient is NOT
compared free-running: a ReLU or pool decision that one fp32 route takes differently from fp64 changes the gradient locally by percents,
for torch's fp32 as for any other.  frozen_chain evaluates the backward chain -- linear once the masks, the pool choices and the signs are
given -- with those decisions taken from the maps a call saved; |g - g64| <= 4 max(E32, 1e-6 max |g64|), E32 the error of the same
chain in torch fp32.  The tap's sums are fp64 sums of exact fp64 terms: at most 512 terms in a thread's chain, 8 levels of tree, then
the level's tiles in one chain -- under 1e4 roundings of 1.1e-16 for every shape the tests use, which is the 1e-12 the check allows.
"""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)     # torchvision's indices of VGG19's convolutions up to relu5_1
POOLS = (4, 9, 18, 27)
TAP_RELUS = (1, 6, 11, 20, 29)                               # relu1_1 .. relu5_1
SLICE_OF = {0: 1, 2: 2, 5: 2, 7: 3, 10: 3, 12: 4, 14: 4, 16: 4, 19: 4, 21: 5, 23: 5, 25: 5, 28: 5}
KEYS = [f"slice{SLICE_OF[i]}.{i}.{what}" for i in CONVS for what in ("weight", "bias")]
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
TAPPED = (0, 2, 4, 8, 12)          # of the 13 convolutions
POOL_BEFORE = (2, 4, 8, 12)


def features(sd, x):
    """The five tapped maps of x under the state dict sd (VGG19's own keys), torchvision's features[0:30] written out"""
    taps = []
    for i in range(30):
        if i in CONVS:
            x = F.conv2d(x, sd[f"slice{SLICE_OF[i]}.{i}.weight"], sd[f"slice{SLICE_OF[i]}.{i}.bias"], padding=1)
        elif i in POOLS:
            x = F.max_pool2d(x, 2, 2)
        else:
            x = F.relu(x)
            if i in TAP_RELUS:
                taps.append(x)
    return taps


def loss(sd, pred, gt):
    """-> (total, [five levels]) in the dtype of the inputs, the reference's operations in its order"""
    fg, fp = features(sd, gt), features(sd, pred)
    total, levels = 0, []
    for i in range(5):
        levels.append(F.l1_loss(fp[i], fg[i]))
        total += WEIGHTS[i] * levels[-1]
    return total, levels


def cast(sd, dtype, device=None):
    return {k: v.detach().to(dtype=dtype, device=device) for k, v in sd.items()}


def seed_c(g, weight, count):
    """c = fp32((g * w_l) / N) with fp32 operands: IEEE operations on the host"""
    return np.float32(np.float32(g) * np.float32(weight)) / np.float32(count)


def route(up, y):
    """up through the adjoint of max_pool2d(relu(y), 2): each element to torch's pick of its window, zeros elsewhere"""
    _, idx = F.max_pool2d(F.relu(y), 2, 2, return_indices=True)
    return F.max_unpool2d(up, idx, 2, 2, output_size=y.shape[-2:])


def join_formula(y, y_gt, up, inv_s, c, pooled):
    """The backward join written out in torch (fp32, each operation rounded once) -> G"""
    v = None
    if up is not None:
        v = up * inv_s
        if pooled:
            v = route(v, y)
    if y_gt is not None:
        s = torch.sign(F.relu(y) - F.relu(y_gt)) * float(c)
        v = s if v is None else v + s
    return torch.where(y <= 0, torch.zeros_like(v), v)


def frozen_chain(sd, saved, g, dtype):
    """The gradient of total to the prediction with every decision (ReLU masks, pool picks, signs) read from the maps `saved` of a
    call (content_loss(..., return_saved=True)); the arithmetic -- the seeds, the thirteen transposed convolutions, the sums -- in
    `dtype` on the maps' device."""
    maps, gts = saved["maps"], saved["gt"]
    W = [sd[k].detach().to(dtype=dtype, device=maps[0].device) for k in KEYS[0::2]]

    def seed(level, k):
        c = (torch.tensor(g, dtype=dtype) * WEIGHTS[level] / maps[k].numel()).item()
        return torch.sign(F.relu(maps[k]) - F.relu(gts[level])).to(dtype) * c

    G = (maps[12] > 0) * seed(4, 12)
    for k in range(12, 0, -1):
        up = F.conv_transpose2d(G, W[k], padding=1)
        if k in POOL_BEFORE:
            up = route(up, maps[k - 1])
        if k - 1 in TAPPED:
            up = up + seed(TAPPED.index(k - 1), k - 1)
        G = (maps[k - 1] > 0) * up
    return F.conv_transpose2d(G, W[0], padding=1)


def rule(name, got, want64, got32, floor=1e-6):
    """The project's rule: |got - want64| <= 4 max(|got32 - want64|, floor * max |want64|), all maxima over the elements.  Prints."""
    want64 = want64.double()
    err = (got.double() - want64).abs().max().item()
    e32 = (got32.double() - want64).abs().max().item()
    bound = 4 * max(e32, floor * want64.abs().max().item())
    print(f"{name}: error {err:.3e} / bound {bound:.3e} = {err / bound:.3f}  (E32 {e32:.3e}, max |ref| {want64.abs().max().item():.3e})")
    return err, bound


def same_bits(a, b):
    """Equal bit for bit, a NaN of one a NaN of the other"""
    a, b = a.contiguous(), b.contiguous()
    nan = torch.isnan(a)
    return a.shape == b.shape and bool((nan == torch.isnan(b)).all()) and torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))
