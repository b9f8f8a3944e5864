"""GPU: the PixelCNN's training kernels (csrc/pixelcnn_train.hip behind include/pixelsynth_pixelcnn_train.h), their autograd Functions
(lmconv/train_ops.py), the route through gated_resnet / OurPixelCNN._forward_layers / likelihood.ar_loss, and lmconv/train.py.

Kernel level: every output against the fp64 formulas of tests/_pixelcnn_train_ref.py inside its DERIVED bounds (its docstring says where
they come from), every gradient under the project's rule |g - g64| <= 4 max(E32, 1e-6 max |g64|); no element is left out.  The shapes
are the ones at which the launch changes: location counts around the wavefront, the workgroup and the threshold between four lanes
and one lane per location (262144), and above it a count that leaves the one-lane form's last workgroup partial with a C of two rounds
of the channel walk and a tail; grids whose L is no multiple of 4; C = 2, 3, 11, 80, 160 (both forms stream the channels: there is no
register form and so no channel limit to stand on either side of).

Network level: PixelSynth's OurPixelCNN on the 2 x 8 x 8 setup of tests/test_lmconv_bwd_gpu.py, whose helpers and constants are
imported, against the fp64 twin oracle.lmconv_oracle.pixelcnn_forward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pixelcnn_train_ref as ref
from oracle import lmconv_oracle as lo
from pixelsynth_amd import _lib
from pixelsynth_amd.lmconv import train_ops
from test_lmconv_bwd_gpu import B8, C_GRAD, H8, L8, W8, _net, _setup, _twin_gradients, val

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIP = train_ops.pixelcnn_train
WORST = {}            # quantity -> the largest error / bound seen in this run (printed by the last test)


def held(name, got, want, bound, quantity):
    r = ref.check(name, got, want, bound)
    WORST[quantity] = max(WORST.get(quantity, 0.0), r)
    assert r <= 1.0, (name, r)


def nhwc(t):
    """t's values in dense (B,H,W,C) storage behind the movedim view nin leaves"""
    return t.movedim(1, -1).contiguous().movedim(-1, 1)


def run_norm_act(x, skip, storage, norm, act, dy):
    """Through train_ops under "hip" -> (y, dx, dskip); the Function must be the one that ran"""
    dx = x.to(DEV).requires_grad_()
    ds = None if skip is None else (nhwc(skip.to(DEV)) if storage == "nhwc" else skip.to(DEV)).requires_grad_()
    with HIP("hip"):
        y = train_ops.norm_act(dx, ds, norm, act)
    assert type(y.grad_fn).__name__ == "_NormActBackward", "the HIP route was not taken"
    y.backward(dy.to(DEV))
    if ds is not None:
        assert ds.grad.stride() == ds.stride(), "the skip's gradient comes back in the skip's storage"
    return y.detach(), dx.grad, None if ds is None else ds.grad


def check_norm_act(name, x, skip, storage, norm, act, dy):
    C = x.shape[1]
    dy = dy if act == "celu" else dy[:, :C]
    y, dx, dskip = run_norm_act(x, skip, storage, norm, act, dy)
    f = ref.norm_act_forward64(x, skip, norm, act)
    held(f"{name} y", y, f["y"], ref.y_bound(x, skip, norm, act, f), "norm_act y")
    fn = lambda a, b: train_ops.norm_act_formula(a, b, norm, act)
    g64, g32 = ref.autograd(fn, (x, skip), dy, torch.float64), ref.autograd(fn, (x, skip), dy, torch.float32)
    closed = ref.norm_act_backward64(x, skip, dy, norm, act)
    assert (closed[0] - g64[0]).abs().max() <= 1e-12 * max(1.0, float(g64[0].abs().max()))
    held(f"{name} dx", dx, g64[0], ref.grad_bound(g32[0], g64[0])[0], "norm_act dx")
    if skip is not None:
        held(f"{name} dskip", dskip, g64[1], ref.grad_bound(g32[1], g64[1])[0], "norm_act dskip")


def stats_of(x):
    """mean, rstd (B,1,H,W) as ps_norm_act_forward_f32 leaves them"""
    B, C, H, W = x.shape
    xd = x.to(DEV)
    y, mean, rstd = torch.empty_like(xd), torch.empty(B, 1, H, W, device=DEV), torch.empty(B, 1, H, W, device=DEV)
    _lib.call("ps_norm_act_forward_f32", xd, None, 0, B, C, H * W, 1, 0, y, mean, rstd)
    return mean, rstd


def check_stats(name, x):
    mean, rstd = stats_of(x)
    m64, r64, xh = ref.pono64(x)
    bm, br = ref.stat_bounds(x, dict(mean=m64, rstd=r64, xh=xh))
    held(f"{name} mean", mean, m64, bm, "mean")
    held(f"{name} rstd", rstd, r64, br, "rstd")


# (B, C, H, W): B L = 1, 63, 64, 65, 255, 256, 257, 262143, 262144 locations (64: a wavefront; 256: a workgroup of one lane per location;
# 262144: from there on a lane owns a location), 105 on the 5 x 7 grid, and 262179 = 1024 * 256 + 35: the one-lane form with a partial
# last workgroup, at C = 11 (two rounds of four channels and a tail of three); C = 2, 3, 11, 80, 160
SHAPES = [(1, 2, 1, 1), (7, 3, 3, 3), (1, 80, 8, 8), (65, 2, 1, 1), (17, 80, 3, 5), (4, 160, 8, 8), (257, 3, 1, 1), (3, 160, 5, 7),
          (29127, 2, 3, 3), (4096, 3, 8, 8), (29131, 11, 3, 3)]
COUNTS = [B * H * W for B, _, H, W in SHAPES]
assert COUNTS == [1, 63, 64, 65, 255, 256, 257, 105, 262143, 262144, 262179] and 262179 % 256 == 35
OPTIONS = [(norm, act, storage) for norm in (True, False) for act in (None, "elu", "celu") for storage in (None, "nchw", "nhwc")
           if norm or act or storage]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_norm_act_against_fp64(shape):
    B, C, H, W = shape
    x, skip, _, dy = ref.inputs(B, C, H, W, seed=C + B)
    assert train_ops.lanes_per_location(B * H * W) == (1 if B * H * W >= ref.WIDE_LOCATIONS else 4)
    check_stats(f"{shape}", x)
    # (every option at the small counts; every fourth at the large ones, and at the largest tensor the three that between them take
    # PONO on and off, every activation and every storage of the skip: the fp64 reference on the host is what takes the time)
    few = [(True, "celu", "nhwc"), (True, None, None), (False, "elu", "nchw")]
    for norm, act, storage in OPTIONS if B * H * W < 60000 else OPTIONS[::4] if B * C * H * W < 2 ** 21 else few:
        check_norm_act(f"{shape} norm={norm} act={act} skip={storage}", x, skip if storage else None, storage, norm, act, dy)


def run_gate(vg, u, dout):
    dvg, du = vg.to(DEV).requires_grad_(), u.to(DEV).requires_grad_()
    with HIP("hip"):
        out = train_ops.gate(dvg, du)
    assert type(out.grad_fn).__name__ == "_GateBackward", "the HIP route was not taken"
    out.backward(dout.to(DEV))
    return out.detach(), dvg.grad, du.grad


def check_gate(name, vg, u, dout):
    out, gvg, gu = run_gate(vg, u, dout)
    f = ref.gate_forward64(vg, u)
    held(f"{name} out", out, f["out"], ref.out_bound(vg, f), "gate out")
    g64, g32 = (ref.autograd(train_ops.gate_formula, (vg, u), dout, dt) for dt in (torch.float64, torch.float32))
    assert (ref.gate_backward64(vg, dout) - g64[0]).abs().max() <= 1e-12 * max(1.0, float(g64[0].abs().max()))
    held(f"{name} dvg", gvg, g64[0], ref.grad_bound(g32[0], g64[0])[0], "gate dvg")
    assert torch.equal(gu.cpu(), dout), "the gradient of u is the incoming one, handed through"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gate_against_fp64(shape):
    B, C, H, W = shape
    x, skip, u, dy = ref.inputs(B, C, H, W, seed=C + B + 1)
    check_gate(f"{shape}", torch.cat([x, skip], 1), u, dy[:, :C])


def test_an_offset_far_larger_than_the_spread():
    """100 + 0.01 randn: the variance, 1e-4, has to come out positive and inside its bound (a sum of squares about 0 in fp32 has no
    digit of it)"""
    for shape in ((2, 80, 8, 8), (3, 3, 5, 7)):
        x, skip, u, dy = ref.inputs(*shape, seed=11, scale="offset")
        check_stats(f"offset {shape}", x)
        _, rstd = stats_of(x)
        assert (rstd > 0).all() and (rstd < 1 / np.sqrt(ref.EPS)).all()
        check_norm_act(f"offset {shape}", x, skip, "nchw", True, "celu", dy)
        check_gate(f"offset {shape}", torch.cat([x, skip], 1), u, dy[:, :shape[1]])


def test_saturated_activations():
    """+-30: elu(-30) = -1 + 9e-14 and its slope 9e-14, the sigmoid within 1e-13 of 0 and of 1"""
    for shape in ((2, 80, 8, 8), (3, 3, 5, 7)):
        x, skip, u, dy = ref.inputs(*shape, seed=12, scale="large")
        for norm, sk in ((False, None), (True, skip), (False, skip)):
            check_norm_act(f"+-30 {shape} norm={norm}", x, sk, "nhwc" if sk is not None else None, norm, "celu", dy)
        check_norm_act(f"+-30 {shape} elu", x, None, None, False, "elu", dy)
        check_gate(f"+-30 {shape}", torch.cat([u, skip], 1), u, dy[:, :shape[1]])     # (the gate's half is +-30)


def test_the_halves_are_where_the_reference_puts_them():
    C, k = 5, 3
    x = torch.zeros(2, C, 3, 3)
    x[:, k] = 1.0
    y, _, _ = run_norm_act(x, None, None, False, "celu", torch.ones(2, 2 * C, 3, 3))
    want = torch.zeros(2, 2 * C, 3, 3, dtype=torch.float64)
    want[:, k], want[:, C + k] = 1.0, np.expm1(-1.0)
    assert (y.cpu().double() - want).abs().max() <= 2 * ref.U, "elu(z) in channels 0 .. C-1, elu(-z) in C .. 2C-1"
    # the gate: only channel k's gate is open, and the value half is what gets normalised
    gen = torch.Generator().manual_seed(2)
    v, u = torch.randn(2, C, 3, 3, generator=gen), torch.randn(2, C, 3, 3, generator=gen)
    g = torch.full((2, C, 3, 3), -30.0)
    g[:, k] = 30.0
    out, _, _ = run_gate(torch.cat([v, g], 1), u, torch.ones_like(u))
    vh = ref.pono64(v)[2]
    d = out.cpu().double() - u.double()
    assert (d[:, k] - vh[:, k]).abs().max() <= 1e-5 and np.abs(np.delete(d.numpy(), k, 1)).max() <= 1e-6


@pytest.mark.parametrize("shape", [(3, 80, 5, 7), (29131, 11, 3, 3)], ids=["four_lanes", "one_lane"])
def test_only_the_skip_wants_a_gradient(shape):
    """dx = NULL: the kernel skips the two sums and writes dskip alone"""
    x, skip, _, dy = ref.inputs(*shape, seed=31)
    dx, ds = x.to(DEV), nhwc(skip.to(DEV)).requires_grad_()
    with HIP("hip"):
        y = train_ops.norm_act(dx, ds, True, "celu")
    assert type(y.grad_fn).__name__ == "_NormActBackward"
    y.backward(dy.to(DEV))
    assert dx.grad is None and ds.grad.stride() == ds.stride()
    fn = lambda a, b: train_ops.norm_act_formula(a, b, True, "celu")
    g64, g32 = ref.autograd(fn, (x, skip), dy, torch.float64), ref.autograd(fn, (x, skip), dy, torch.float32)
    held(f"{shape} dskip alone", ds.grad, g64[1], ref.grad_bound(g32[1], g64[1])[0], "norm_act dskip")


# ------------------------------------------------------------------------------------------------------------- the loss's backward
FR, LR = 3, 35      # three frames of a 5 x 7 grid: frame 0 mixed, frame 1 all sampled, frame 2 all observed


def _loss_case(layout, seed=0):
    gen = torch.Generator().manual_seed(seed)
    logits = 3.0 * torch.randn(FR, 512, 5, 7, generator=gen)
    targets = torch.randint(0, 512, (FR, LR), generator=gen)
    region = torch.zeros(FR, LR, dtype=torch.uint8)
    region[0, ::3], region[1] = 1, 1
    dl = (nhwc(logits.to(DEV)) if layout == "lc" else logits.to(DEV)).requires_grad_()
    assert dl.is_contiguous() == (layout == "chw")
    return logits, targets, region, dl


@pytest.mark.parametrize("T", [1.0, 0.7])
@pytest.mark.parametrize("group", ["all", "sampled", "observed"])
@pytest.mark.parametrize("layout", ["chw", "lc"])
def test_code_nll_backward(layout, group, T):
    from pixelsynth_amd.likelihood import code_nll
    logits, targets, region, dl = _loss_case(layout)
    with HIP("hip"):
        loss = train_ops.code_cross_entropy(dl, targets.to(DEV), region.to(DEV), group, T)
    assert type(loss.grad_fn).__name__ == "_CodeCrossEntropyBackward" and loss.dim() == 0 and loss.dtype == torch.float32
    rows = dl.detach() if layout == "chw" else dl.detach().movedim(1, -1).reshape(FR, LR, 512)
    score = code_nll(rows, targets.to(DEV), region.to(DEV), T, layout)
    assert val(loss) == float(score.mean_nll(group).float()), "the value is sum nll / count of the fp64 sums"
    (loss * 2.5).backward()
    grad = dl.grad
    assert grad.stride() == dl.stride() and grad.data_ptr() != dl.data_ptr(), "the gradient comes back in the logits' own storage"
    fn = lambda t: train_ops.cross_entropy_formula(t, targets, region, group, T)
    g64, = ref.autograd(fn, (logits,), torch.tensor(2.5), torch.float64)
    g32, = ref.autograd(fn, (logits,), torch.tensor(2.5), torch.float32)
    assert (ref.code_nll_backward64(logits.reshape(FR, 512, LR), targets, region, group, T, 2.5).reshape(g64.shape) - g64).abs().max() <= 1e-12
    held(f"{layout} {group} T={T} grad_logits", grad, g64, ref.grad_bound(g32, g64)[0], "grad_logits")
    take = ref.group_mask(region, group, targets).reshape(FR, 1, 5, 7).expand_as(logits)
    outside = grad.cpu()[~take]
    assert not outside.any() and not torch.signbit(outside).any(), "rows outside the group are +0"
    if group != "all":
        assert not grad[2 if group == "sampled" else 1].any(), "a frame without a location of the group gets zeros"
        assert grad[1 if group == "sampled" else 2].abs().sum(0).min() > 0, "a frame that is one group whole gets every row"
    # a row sums to 0: each entry is scale (p - [c = t]), sum |entries| <= 2 scale, the fp32 sum of the exponentials is a tree 12 deep
    # and the division, the subtraction and the product round once each: 16 u of 2 scale, and the fp64 sum here adds nothing
    scale = 2.5 / T / int(ref.group_mask(region, group, targets).sum())
    assert grad.double().sum(1).abs().max().item() <= 32 * ref.U * scale


@pytest.mark.parametrize("layout", ["chw", "lc"])
def test_code_nll_backward_nan_rows(layout):
    logits, targets, region, _ = _loss_case(layout, seed=1)
    targets[0, 0], targets[0, 3], targets[1, 5] = -1, 512, 7            # 0,0 and 0,3: sampled (bad targets); 0,1 observed
    targets[0, 1] = -1                                                   # a bad target outside the group: no NaN there
    logits[1, 9, 1, 0] = float("nan")                                    # location 7 of frame 1 (sampled)
    dl = (nhwc(logits.to(DEV)) if layout == "lc" else logits.to(DEV)).requires_grad_()
    with HIP("hip"):
        loss = train_ops.code_cross_entropy(dl, targets.to(DEV), region.to(DEV), "sampled", 1.0)
    assert torch.isnan(loss)                                             # (as the forward gives those locations a NaN)
    loss.backward()
    rows = dl.grad.cpu().reshape(FR, 512, LR)
    bad = torch.zeros(FR, LR, dtype=torch.bool)
    bad[0, 0] = bad[0, 3] = bad[1, 7] = True
    assert torch.isnan(rows.movedim(1, -1)[bad]).all(), "a target of -1, of 512 and a NaN logit each give a row of NaN"
    assert torch.isfinite(rows.movedim(1, -1)[~bad]).all() and not rows[0, :, 1].any()


# -------------------------------------------------------------------------------------------------------------------- determinism
def _bits(x, skip, u, dy):
    """Every output of the two kernel families for these operands"""
    C = x.shape[1]
    return run_norm_act(x, skip, "nhwc", True, "celu", dy) + run_gate(torch.cat([x, skip], 1), u, dy[:, :C])[:2] + stats_of(x)


def test_two_runs_and_a_frame_alone_give_the_same_bits():
    x, skip, u, dy = ref.inputs(3, 80, 5, 7, seed=21)
    first, again = _bits(x, skip, u, dy), _bits(x, skip, u, dy)
    assert all(torch.equal(p, q) for p, q in zip(first, again))
    alone = _bits(x[1:2], skip[1:2], u[1:2], dy[1:2])
    assert all(torch.equal(p[1:2], q) for p, q in zip(first, alone)), "frame 1 of 3 against the frame alone"
    logits, targets, region, dl = _loss_case("lc")
    grads = []
    for _ in range(2):
        dl.grad = None
        with HIP("hip"):
            train_ops.code_cross_entropy(dl, targets.to(DEV), region.to(DEV), "sampled", 0.7).backward()
        grads.append(dl.grad.clone())
    assert torch.equal(*grads)


def test_one_lane_and_four_lanes_per_location_give_the_same_bits():
    """64 frames of 64 x 64 are 262144 locations: a lane each; frame 5 alone is 4096: four lanes each.  The chains are the same.
    C = 22: five full rounds of the channel walk (the unrolled four and one more) and a tail of two, chains of 6, 6, 5 and 5 terms --
    a one-lane form that added its channels as one sequence, or a chain in another order, rounds differently somewhere in 262144 sums."""
    x, skip, u, dy = ref.inputs(64, 22, 64, 64, seed=22)
    assert train_ops.lanes_per_location(64 * 4096) == 1 and train_ops.lanes_per_location(4096) == 4
    wide, narrow = _bits(x, skip, u, dy), _bits(x[5:6], skip[5:6], u[5:6], dy[5:6])
    assert all(torch.equal(p[5:6], q) for p, q in zip(wide, narrow))
    # The outputs above are fp64 sums rounded once, which hides the order of the additions (another order moves an fp32 result once in
    # 10^9).  So the order itself on values where it shows in every location: the mean has to be the bits of the header's four chains
    # evaluated on the host, on both forms -- one sequential chain would lose the small values between the +-2^60.
    xs = ref.order_sensitive(64, 22, 64, 64, seed=23)
    want = ref.chained_mean(xs)
    plain = xs.double().sum(1, keepdim=True).div(22).float()
    assert (want != plain).float().mean() > 0.9, "the input must tell the orders apart"
    (mean_w, rstd_w), (mean_n, rstd_n) = stats_of(xs), stats_of(xs[5:6])
    assert torch.equal(mean_w.cpu(), want), "one lane per location: the four chains of the header, bit for bit"
    assert torch.equal(mean_n.cpu(), want[5:6]), "four lanes per location: the same"
    assert torch.equal(rstd_w[5:6], rstd_n) and torch.isfinite(rstd_w).all()


# ------------------------------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("skip", [0, 1])
def test_a_gated_block_against_its_fp64_twin(skip):
    """gated_resnet(80) on 2 x 8 x 8 under "hip".  The new kernels inside the block are held to their DERIVED forward bounds on the
    operands they actually got: what conv_input and nin_skip handed to norm_act, and what conv_out handed to the gate, each against the
    fp64 formula on those fp32 tensors (y_bound, out_bound).  Beside that the whole block against oracle.lmconv_oracle.gated_resnet in
    fp64: the output and every gradient under the gradient rule, 4 max(E32, 1e-6 max |fp64|) with E32 the twin's own fp32 error (the
    masked convolutions are part of both, so for the whole block no bound tighter than the twin's own error can be derived)."""
    from pixelsynth_amd.lmconv.layers import PONO, gated_resnet
    from pixelsynth_amd.lmconv.locally_masked_convolution import locally_masked_conv2d
    from pixelsynth_amd.lmconv.utils import concat_elu
    torch.manual_seed(skip)
    block = gated_resnet(80, lambda ci, co: locally_masked_conv2d(ci, co), lambda n: PONO(), concat_elu, skip_connection=skip, dropout_prob=0.0)
    mask = _setup()[0][1]
    gen = torch.Generator().manual_seed(5 + skip)
    u, a, g = (torch.randn(B8, 80, H8, W8, generator=gen) for _ in range(3))
    names = [k for k, _ in block.named_parameters()]
    sd = {k: v.detach().clone() for k, v in block.named_parameters()}

    def twin(dtype):
        leaves = {k: v.to(dtype).requires_grad_() for k, v in sd.items()}
        tu, ta = u.to(dtype).requires_grad_(), a.to(dtype).requires_grad_()
        out = lo.gated_resnet(leaves, "", tu, ta if skip else None, mask.to(dtype))
        grads = torch.autograd.grad(out, [tu] + ([ta] if skip else []) + [leaves[k] for k in names], g.to(dtype))
        return [out.detach()] + list(grads)
    t64, t32 = twin(torch.float64), twin(torch.float32)
    block = block.to(DEV)
    du, da = u.to(DEV).requires_grad_(), a.to(DEV).requires_grad_()
    seen = {}
    hooks = [block.conv_input.register_forward_hook(lambda m, i, o: seen.update(h=o.detach().cpu())),
             block.conv_out.register_forward_hook(lambda m, i, o: seen.update(celu=i[0].detach(), vg=o.detach().cpu()))]
    if skip:
        hooks.append(block.nin_skip.register_forward_hook(lambda m, i, o: seen.update(skip=o.detach().cpu())))
    with HIP("hip"):
        out = block(du, da if skip else None, mask=mask.to(DEV))
    for h in hooks:
        h.remove()
    assert type(out.grad_fn).__name__ == "_GateBackward"
    f = ref.norm_act_forward64(seen["h"], seen.get("skip"), True, "celu")
    held(f"block skip={skip} norm_act inside", seen["celu"], f["y"], ref.y_bound(seen["h"], seen.get("skip"), True, "celu", f), "norm_act y")
    f = ref.gate_forward64(seen["vg"], u)
    held(f"block skip={skip} gate inside", out, f["out"], ref.out_bound(seen["vg"], f), "gate out")
    grads = torch.autograd.grad(out, [du] + ([da] if skip else []) + [p for _, p in block.named_parameters()], g.to(DEV))
    labels = ["out", "og_x"] + (["a"] if skip else []) + names
    for label, got, w64, w32 in zip(labels, [out] + list(grads), t64, t32):
        held(f"block skip={skip} {label}", got, w64, ref.grad_bound(w32, w64)[0], "block " + ("out" if label == "out" else "gradients"))


# -------------------------------------------------------------------------------------------------------------------- the network
_TWIN = {}


def _twin(dtype):
    if dtype not in _TWIN:
        _TWIN[dtype] = _twin_gradients(dtype)
    return _TWIN[dtype]


def _device_setup():
    masks, codes, region = _setup()
    return [m.to(DEV) for m in masks], codes.to(DEV), region.to(DEV)


def test_parameter_gradients_against_the_fp64_twin_under_hip():
    from pixelsynth_amd.likelihood import ar_loss
    dm, dc, dr = _device_setup()
    net = _net()
    with HIP("hip"):
        loss = ar_loss(net, dc, dm, region=dr)
    assert type(loss.grad_fn).__name__ == "_CodeCrossEntropyBackward"
    loss.backward()
    (l64, g64), (l32, g32) = _twin(torch.float64), _twin(torch.float32)
    got = {k: p.grad for k, p in net.named_parameters()}
    assert set(got) == set(g64) and all(v is not None for v in got.values())
    err = lambda g, k: float((g[k].detach().cpu().double() - g64[k]).abs().max() / g64[k].abs().max())
    e_twin, e_hip = {k: err(g32, k) for k in g64}, {k: err(got, k) for k in g64}
    E = max(e_twin.values())
    worst = max(e_hip, key=e_hip.get)
    print(f"loss: HIP route {val(loss):.6f} twin fp32 {l32:.6f} fp64 {l64:.6f}")
    print(f"twin fp32: E = max e_k {E:.3e}; HIP route: max e_k {e_hip[worst]:.3e} ({worst}); largest e_k(HIP) / E = {e_hip[worst] / E:.3f}")
    WORST["network e_k / E (bound C_GRAD = 4)"] = e_hip[worst] / E
    assert all(e <= C_GRAD * E for e in e_hip.values()), (worst, e_hip[worst] / E)


def test_ar_loss_under_hip_is_the_engine_score_and_the_torch_route():
    from pixelsynth_amd.likelihood import ar_loss, score_codes
    dm, dc, dr = _device_setup()
    net = _net()
    with torch.no_grad():
        logits = net.engine(H8, W8, B8).forward(dc, *dm)
        score, cool = score_codes(net, dc, dm, region=dr), score_codes(net, dc, dm, region=dr, temperature=0.7)
    tol = 2 * (1e-4 + 1e-4 * float(logits.abs().max()))
    for group in ("sampled", "all", "observed"):
        with HIP("hip"):
            hip = ar_loss(net, dc, dm, region=dr, group=group)
        with HIP("torch"):
            plain = ar_loss(net, dc, dm, region=dr, group=group)
        assert hip.dim() == 0 and hip.dtype == torch.float32 and hip.requires_grad and hip.is_cuda
        print(f"{group}: hip {val(hip):.6f} torch {val(plain):.6f} engine {float(score.mean_nll(group)):.6f} tolerance {tol:.2e}")
        assert abs(val(hip) - float(score.mean_nll(group))) <= tol, group
        assert abs(val(hip) - val(plain)) <= 1e-5 * abs(val(plain)), group
    with HIP("hip"):
        assert abs(val(ar_loss(net, dc, dm, region=dr, temperature=0.7)) - float(cool.mean_nll("sampled"))) <= tol / 0.7

    class Opt:
        pixelcnn_train = "hip"

    class Model:            # what ar_loss takes of a ZbufferModelPts: its PixelCNN and its options
        outpaint2, opt = net, Opt()
    assert type(ar_loss(Model(), dc, dm, region=dr).grad_fn).__name__ == "_CodeCrossEntropyBackward"
    assert type(ar_loss(net, dc, dm, region=dr).grad_fn).__name__ != "_CodeCrossEntropyBackward", "the default is the torch route"


def test_the_hip_route_runs_none_of_the_torch_passes(monkeypatch):
    from pixelsynth_amd.likelihood import ar_loss
    dm, dc, dr = _device_setup()
    net = _net()
    real = {"elu": F.elu, "var_mean": torch.var_mean, "sigmoid": torch.sigmoid, "cat": torch.cat, "cross_entropy": F.cross_entropy}
    hits = dict.fromkeys(real, 0)

    def spy(name, fail):
        def f(*args, **kwargs):
            if fail:
                raise AssertionError(f"{name} ran under the HIP route")
            hits[name] += 1
            return real[name](*args, **kwargs)
        return f
    for fail in (True, False):
        for name in real:
            monkeypatch.setattr(F if name in ("elu", "cross_entropy") else torch, name, spy(name, fail))
        net.zero_grad()
        with HIP("hip" if fail else "torch"):
            ar_loss(net, dc, dm, region=dr).backward()
        assert all(p.grad is not None for p in net.parameters())
    assert all(n > 0 for n in hits.values()), hits


def test_ten_train_steps_under_hip_reach_the_rebuilt_engine():
    from pixelsynth_amd.likelihood import score_codes
    from pixelsynth_amd.lmconv.train import train_step
    dm, dc, dr = _device_setup()
    net = _net()
    with torch.no_grad():
        start = float(score_codes(net, dc, dm, region=dr).mean_nll("sampled"))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    with HIP("hip"):
        for _ in range(10):
            loss, bits, norm = train_step(net, opt, dc, dm, region=dr, group="sampled")
    assert norm is None and loss.is_cuda and loss.dim() == 0 and not loss.requires_grad
    assert abs(val(bits) - val(loss) / np.log(2.0)) <= 1e-6 * val(bits)
    with torch.no_grad():
        end = float(score_codes(net, dc, dm, region=dr).mean_nll("sampled"))
    print(f"engine mean_nll(sampled): {start:.4f} before, {end:.4f} after ten train_steps under hip")
    assert end < 0.5 * start


def test_train_step_clips_the_gradient():
    from pixelsynth_amd.lmconv.train import train_step
    dm, dc, dr = _device_setup()
    net = _net()
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    with HIP("hip"):
        loss, bits, norm = train_step(net, opt, dc, dm, region=dr, clip=0.1)
    assert norm is not None and norm.is_cuda and norm.dim() == 0 and val(norm) > 0.1
    after = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters())))
    print(f"gradient norm {val(norm):.4f} before clipping, {after:.6f} after (clip 0.1)")
    # clip_grad_norm_ scales by clip / (norm + 1e-6) in fp32: the norm after is 0.1 (1 - 1e-6 / norm) within a few roundings
    assert abs(after - 0.1) <= 0.1 * (1e-6 / val(norm) + 8 * ref.U)


def test_zz_report():
    """The largest error / bound per quantity of this run (README, docs/LAB_NOTEBOOK.md)"""
    for k in sorted(WORST):
        print(f"WORST {k}: {WORST[k]:.3f}")
