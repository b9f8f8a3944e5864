"""GPU: the depth Unet's training kernels (csrc/unet_train.hip, networks/unet_train.py) and its route (Unet._forward_hip,
conv_routes._unet_train_conv, training.hip_routes_with_unet) against the fp64 mirrors and bounds of tests/_unet_train_ref.py.

  bn_act_train   statistics, y, z, dx, dweight, dbias at every shape of ref.BN_SHAPES with and without the slope and with dy, dz or both;
                 an ill-conditioned variance; a planted NaN; the running statistics after one and two calls; N = 1 and eval() on torch
  relu_up2_cat   forward and both adjoints at ref.UP_SHAPES x ref.UP_CHANNELS and (256, 256) at 2 x 2; one-hot operands; NaN; a frame
                 alone against frame 1 of 3; every output twice
  conv route     which convolution reaches which Function
  networks       Unet(4) on 2 x 256 x 256 and Unet(32) on 1 x 256 x 256 against their fp64 twins on the host, spectral norm on, cudnn off.
                 The twins take the HIP run's own ReLU / leaky ReLU decisions (ref.Decisions): at these sizes a few of the 10^6 .. 10^7
                 activations lie at rounding distance from 0 in any fp32 run, and one decision flipped moves a gradient by more than the
                 roundings the rule allows for.  The count of decisions that differ from the twin's own signs is printed.
  training       ten Adam steps of Unet(4) on an L1 depth target; one BaseModel step against hip_routes_with_spectral()

Measured on the MI355X (largest error / bound per quantity; first and last loss): README, "The depth Unet's training step".
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _forward_train_util as U
import _unet_train_ref as ref
from pixelsynth_amd import _lib, training
from pixelsynth_amd.base_model import BaseModel
from pixelsynth_amd.networks import architectures as arch, f16x3, thin_train, unet_train as UT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def bn_module(weight, bias):
    mod = nn.BatchNorm2d(weight.numel()).train()
    with torch.no_grad():
        mod.weight.copy_(weight), mod.bias.copy_(bias)
    return mod.to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def library_stats(x):
    """mean, var of the library on x (B, C, H, W) on the host, without a module"""
    xg = nhwc(x)
    B, C, H, W = x.shape
    ws = torch.empty(_lib.call("ps_unet_train_workspace_bytes", B * H * W, C), dtype=torch.uint8, device=DEV)
    mean, var, rstd = (torch.empty(C, device=DEV) for _ in range(3))
    _lib.call("ps_bn_stats_f32", xg, B * H * W, C, EPS, 0.1, None, None, None, mean, var, rstd, ws, ws.numel())
    return mean, var


def bn_run(x, weight, bias, slope, dy, dz):
    """One forward + backward through the Function -> (y, z, dx, dweight, dbias, module)"""
    mod, xg = bn_module(weight, bias), nhwc(x).requires_grad_()
    with UT.unet_train("hip"):
        out = UT.bn_act_train(xg, mod, slope)
    y, z = (out, None) if slope is None else out
    assert type(y.grad_fn).__name__ == "_BnActBackward" and y.is_contiguous(memory_format=torch.channels_last)
    loss = 0
    if dy is not None:
        loss = loss + (y * dy.to(DEV)).sum()
    if dz is not None:
        loss = loss + (z * dz.to(DEV)).sum()
    loss.backward()
    return y.detach(), None if z is None else z.detach(), xg.grad, mod.weight.grad, mod.bias.grad, mod


@pytest.mark.parametrize("shape", ref.BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_act_train_against_fp64(shape):
    B, H, W, C = shape
    x, weight, bias, dy, dz = ref.bn_inputs(B, H, W, C, seed=B + H + W + C)
    f = ref.bn_forward64(x, weight, bias, EPS, ref.SLOPE)
    assert (f["y"].abs() > ref.forward_bound(x, f)).all(), "a decision of the leaky ReLU is in doubt in fp32: pick another seed"
    mean, var = library_stats(x)
    bm, bv = ref.stat_bounds(x, rows=B * H * W)
    worst = max(ref.check(f"{shape} mean", mean, f["mean"], bm), ref.check(f"{shape} var", var, f["var"], bv))
    keep, share = ref.kink_free(f["y"])
    print(f"{shape} share of elements within {ref.KINK} of the kink: {share:.2e}")
    assert share <= ref.KINK_SHARE
    for slope, gy, gz in ((None, dy, None), (ref.SLOPE, dy, None), (ref.SLOPE, None, dz), (ref.SLOPE, dy, dz)):
        tag = f"{shape} slope {slope} dy {gy is not None} dz {gz is not None}"
        y, z, dx, dw, db, _ = bn_run(x, weight, bias, slope, gy, gz)
        again = bn_run(x, weight, bias, slope, gy, gz)
        assert all(same_bits(s, t) for s, t in zip((y, z, dx, dw, db), again) if s is not None), tag + ": two runs differ"
        worst = max(worst, ref.check(tag + " y", y, f["y"], ref.forward_bound(x, f)))
        if slope is not None:
            worst = max(worst, ref.check(tag + " z", z, f["z"], ref.z_bound(x, f)))
        want = ref.bn_backward64(x, gy, gz, weight, bias, EPS, slope)
        g32 = ref.bn_autograd(x, weight, bias, gy, gz, EPS, slope if slope is not None else 1.0, torch.float32)
        sel = keep if gz is not None else torch.ones_like(keep)
        for name, got, w64, w32 in zip(("dx", "dweight", "dbias"), (dx, dw, db), want, g32):
            if name == "dx":
                got, w64, w32 = got.cpu()[sel], w64[sel], w32[sel]
            bound, _ = ref.grad_bound(w32, w64)
            worst = max(worst, ref.check(f"{tag} {name}", got, w64, bound))
    assert worst <= 1.0


def test_bn_variance_where_fp32_cancels():
    """100 + 0.01 randn: the fp64 sums keep the variance inside its bound; the fp32 m2 - m^2 of the same data is far outside"""
    B, H, W, C = 2, 16, 16, 32
    x, weight, bias, _, _ = ref.bn_inputs(B, H, W, C, seed=3, offset=100.0, spread=0.01)
    f = ref.bn_forward64(x, weight, bias, EPS, ref.SLOPE)
    mean, var = library_stats(x)
    bm, bv = ref.stat_bounds(x, rows=B * H * W)
    assert ref.check("ill-conditioned mean", mean, f["mean"], bm) <= 1.0 and ref.check("ill-conditioned var", var, f["var"], bv) <= 1.0
    naive = (x * x).mean((0, 2, 3)) - x.mean((0, 2, 3)) ** 2
    assert ref.check("fp32 m2 - m^2", naive, f["var"], bv) > 10.0
    y, z, *_ = bn_run(x, weight, bias, ref.SLOPE, torch.ones_like(x), None)
    assert ref.check("ill-conditioned y", y, f["y"], ref.forward_bound(x, f)) <= 1.0
    assert ref.check("ill-conditioned z", z, f["z"], ref.z_bound(x, f)) <= 1.0


def test_bn_keeps_a_nan():
    x, weight, bias, dy, _ = ref.bn_inputs(3, 5, 7, 12, seed=4)
    x[1, 5, 2, 3] = float("nan")
    y, z, *_ = bn_run(x, weight, bias, ref.SLOPE, dy, None)
    for t in (y, z):
        bad = torch.isnan(t)
        assert bad[:, 5].all() and not bad[:, :5].any() and not bad[:, 6:].any() and torch.isfinite(t[:, :5]).all()


def test_bn_running_statistics_after_one_and_two_calls():
    worst = 0.0
    for shape in ((3, 5, 7, 12), (1, 1, 2, 4), (1, 1, 257, 4)):
        B, H, W, C = shape
        x1, weight, bias, _, _ = ref.bn_inputs(B, H, W, C, seed=11)
        x2 = ref.bn_inputs(B, H, W, C, seed=12, offset=-0.7, spread=0.5)[0]
        mod = bn_module(weight, bias)
        for calls, x in enumerate((x1, x2), 1):
            rm, rv = mod.running_mean.clone(), mod.running_var.clone()
            versions = (mod.running_mean._version, mod.running_var._version, mod.num_batches_tracked._version)
            with UT.unet_train("hip"), torch.no_grad():
                UT.bn_act_train(nhwc(x), mod, ref.SLOPE if calls == 1 else None)
            rm64, rv64, bm, bv = ref.running64(rm, rv, x, mod.momentum)
            worst = max(worst, ref.check(f"{shape} running_mean after {calls}", mod.running_mean, rm64, bm),
                        ref.check(f"{shape} running_var after {calls}", mod.running_var, rv64, bv))
            assert int(mod.num_batches_tracked) == calls and mod.num_batches_tracked.dtype == torch.int64
            assert all(v > w for v, w in zip((mod.running_mean._version, mod.running_var._version, mod.num_batches_tracked._version), versions))
    assert worst <= 1.0


def test_bn_one_value_and_eval_reach_torch(monkeypatch):
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    _, weight, bias, _, _ = ref.bn_inputs(1, 1, 1, 4)
    mod, seen = bn_module(weight, bias), []
    mod.register_forward_pre_hook(lambda m, args: seen.append(tuple(args[0].shape)))
    one = nhwc(torch.randn(1, 4, 1, 1))
    with UT.unet_train("hip"):
        assert not UT.takes_bn(one, mod)
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            UT.bn_act_train(one, mod, ref.SLOPE)
        x = nhwc(torch.randn(2, 4, 3, 3))
        assert UT.takes_bn(x, mod) and not UT.takes_bn(x, mod.eval())
        tracked = int(mod.num_batches_tracked)          # (torch counts the batch it then refuses)
        y, z = UT.bn_act_train(x, mod, ref.SLOPE)
        assert same_bits(y, F.batch_norm(x, mod.running_mean, mod.running_var, mod.weight, mod.bias, False, 0.1, EPS))
        assert same_bits(z, F.leaky_relu(y, ref.SLOPE)) and int(mod.num_batches_tracked) == tracked
    assert seen == [(1, 4, 1, 1), (2, 4, 3, 3)] and not calls
    mod.train()
    assert not calls and UT.bn_act_train(x, mod).grad_fn is not None and not calls       # the default route is torch's
    for refused in (x.double(), x.contiguous(), x.cpu()):
        assert not UT.takes_bn(refused, mod)


# ---------------------------------------------------------------------------------------------------------------------------- relu_up2_cat
def up_inputs(B, H, W, Ca, Cb, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(B, Ca, H, W, generator=gen)
    b = None if Cb is None else torch.randn(B, Cb, H, W, generator=gen)
    g = torch.randn(B, Ca + (Cb or 0), 2 * H, 2 * W, generator=gen)
    return a, b, g


def up_run(a, b, g):
    ag = nhwc(a).requires_grad_()
    bg = None if b is None else nhwc(b).requires_grad_()
    with UT.unet_train("hip"):
        out = UT.relu_up2_cat(ag, bg)
    assert type(out.grad_fn).__name__ == "_ReluUp2CatBackward" and out.is_contiguous(memory_format=torch.channels_last)
    (out * g.to(DEV)).sum().backward()
    return out.detach(), ag.grad, None if b is None else bg.grad


UP_CASES = [(s, c) for s in ref.UP_SHAPES for c in ref.UP_CHANNELS] + [ref.UP_WIDE]


@pytest.mark.parametrize("shape,channels", UP_CASES, ids=lambda v: "x".join(str(i) for i in v))
def test_relu_up2_cat_against_fp64(shape, channels):
    (B, H, W), (Ca, Cb) = shape, channels
    a, b, g = up_inputs(B, H, W, Ca, Cb, seed=H * 100 + W * 10 + Ca)
    out, da, db = up_run(a, b, g)
    again = up_run(a, b, g)
    assert all(same_bits(s, t) for s, t in zip((out, da, db), again) if s is not None), "two runs differ"
    assert out.shape == (B, Ca + (Cb or 0), 2 * H, 2 * W)
    want, mag = ref.up_forward64(a, b)
    tag = f"{shape} {channels}"
    worst = ref.check(tag + " out", out, want, 1.01 * 4 * ref.U * mag + 1e-300)
    if H == W == 1:
        assert same_bits(out.cpu(), F.relu(ref.up_cat(a, b)).expand(-1, -1, 2, 2).contiguous())
    g32 = ref.up_autograd(a, b, g, torch.float32)
    c0 = 0
    for name, src, got, w32 in zip(("da", "db"), (a, b), (da, db), g32):
        if src is None:
            continue
        w64, mag, k = ref.up_adjoint64(g, src, c0)
        c0 += src.size(1)
        keep, share = ref.kink_free(src)
        print(f"{tag} {name}: share of elements within {ref.KINK} of the kink {share:.2e}")
        assert share <= ref.KINK_SHARE
        assert same_bits(got.cpu()[src <= 0], torch.zeros_like(src)[src <= 0])
        worst = max(worst, ref.check(f"{tag} {name} adjoint", got.cpu()[keep], w64[keep], (1.01 * ref.U * k * mag + 1e-300)[keep]))
        bound, _ = ref.grad_bound(w32[keep], w64[keep])
        worst = max(worst, ref.check(f"{tag} {name} rule", got.cpu()[keep], w64[keep], bound))
    assert worst <= 1.0


def test_relu_up2_cat_one_hot_gives_the_weights_exactly():
    H, W = 4, 5
    My, Mx = ref.up_matrix(H).float(), ref.up_matrix(W).float()
    for h, w in ((0, 0), (0, 2), (1, 2), (3, 0), (3, 4), (2, 4)):           # corners, edges, interior
        a, b = torch.zeros(1, 4, H, W), torch.zeros(1, 8, H, W)
        a[0, 1, h, w], b[0, 6, h, w] = 1.0, 2.0
        with UT.unet_train("hip"):
            out = UT.relu_up2_cat(nhwc(a), nhwc(b)).cpu()
        want = torch.zeros(1, 12, 2 * H, 2 * W)
        want[0, 1], want[0, 4 + 6] = torch.outer(My[:, h], Mx[:, w]), 2 * torch.outer(My[:, h], Mx[:, w])
        assert same_bits(out, want), (h, w)
    ones_a, ones_b = torch.ones(1, 4, H, W), torch.ones(1, 8, H, W)
    for p, q in ((0, 0), (0, 5), (3, 4), (7, 0), (7, 9), (4, 9), (1, 1)):
        g = torch.zeros(1, 12, 2 * H, 2 * W)
        g[0, 2, p, q], g[0, 4 + 3, p, q] = 1.0, -3.0
        _, da, db = up_run(ones_a, ones_b, g)
        wa, wb = torch.zeros(1, 4, H, W), torch.zeros(1, 8, H, W)
        wa[0, 2], wb[0, 3] = torch.outer(My[p], Mx[q]), -3 * torch.outer(My[p], Mx[q]) + 0.0       # (+ 0.0: no -0)
        assert same_bits(da.cpu(), wa) and same_bits(db.cpu(), wb), (p, q)


def test_relu_up2_cat_keeps_a_nan_and_masks_what_is_negative():
    a, b, g = up_inputs(1, 8, 8, 4, 4, seed=9)
    a[0, 1, 3, 4] = float("nan")
    out, da, db = up_run(a, b, g)
    bad = torch.isnan(out.cpu())
    My = ref.up_matrix(8)
    rows, cols = (My[:, 3] > 0).nonzero().flatten(), (My[:, 4] > 0).nonzero().flatten()
    assert bad[0, 1][rows][:, cols].all(), "relu dropped the NaN"
    near = torch.zeros(16, 16, dtype=torch.bool)
    near[rows.min() - 1:rows.max() + 2, cols.min() - 1:cols.max() + 2] = True      # (a neighbour of weight 0 is still multiplied, as in torch)
    assert not bad[0, 1][~near].any() and not bad[0, [0, 2, 3, 4, 5, 6, 7]].any()
    assert same_bits(db.cpu()[b <= 0], torch.zeros_like(b)[b <= 0]) and (db.cpu()[b > 0] != 0).all()
    want, mag = ref.up_forward64(torch.nan_to_num(a), b)
    ok = ~bad
    assert ((out.cpu().double() - want).abs()[ok] <= (1.01 * 4 * ref.U * mag)[ok]).all()


def test_relu_up2_cat_a_frame_alone_is_frame_1_of_3():
    a, b, g = up_inputs(3, 16, 16, 8, 12, seed=10)
    out, da, db = up_run(a, b, g)
    o1, da1, db1 = up_run(a[1:2], b[1:2], g[1:2])
    assert same_bits(out[1:2], o1) and same_bits(da[1:2], da1) and same_bits(db[1:2], db1)


# ------------------------------------------------------------------------------------------------------------------------------ the route
def make_unet(f, seed=0):
    torch.manual_seed(seed)
    return arch.Unet(num_filters=f, channels_in=3, channels_out=3, opt=U.train_opts()).train()


def test_which_convolution_reaches_which_function(monkeypatch):
    wide, thin = [], []
    real_wide, real_thin = f16x3.conv3x3_train, thin_train.conv_thin_out_train
    monkeypatch.setattr(f16x3, "conv3x3_train", lambda x, w, b=None: (wide.append((x.size(1), w.size(0), x.size(2))), real_wide(x, w, b))[1])
    monkeypatch.setattr(thin_train, "conv_thin_out_train", lambda x, w, b=None: (thin.append((x.size(1), w.size(0), x.size(2))), real_thin(x, w, b))[1])
    net, x = make_unet(32).to(DEV), torch.randn(1, 3, 256, 256, device=DEV)
    with training.hip_routes_with_unet() as forced:
        assert forced["unet_train"] == "hip" and forced["spectral_train"] == "hip"
        y = net(x)
    assert wide == [(512, 256, 16), (512, 128, 32), (256, 64, 64)] and thin == [(64, 3, 256)]
    assert y.shape == (1, 3, 256, 256) and torch.isfinite(y).all()
    del wide[:], thin[:]
    with UT.unet_train("hip"):                   # the switch alone: not decoder_conv_train, not decoder_thin_train
        net(x)
        assert len(wide) == 3 and len(thin) == 1
        del wide[:], thin[:]
        with torch.no_grad():
            net(x)
        with f16x3.decoder_conv("fp32"):
            net(x)
        small = make_unet(4).to(DEV)
        small(x)
    with UT.unet_train("torch"):
        net(x)
    with training.hip_routes_with_spectral():
        net(x)
    assert not wide and not thin


def graph_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


@pytest.mark.parametrize("filters,batch", [(4, 2), (32, 1)])
def test_network_against_its_fp64_twin(filters, batch, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "enabled", False)
    host = make_unet(filters, seed=filters)
    gen = torch.Generator().manual_seed(7)
    x, G = torch.randn(batch, 3, 256, 256, generator=gen), torch.randn(batch, 3, 256, 256, generator=gen)
    net = copy.deepcopy(host).to(DEV)
    # the HIP run, its decisions recorded in the twin's order: the leaky ReLU behind conv1, those behind the six norms, the eight ReLUs
    seen = ref.Decisions()
    real_leaky, real_bn, real_up = F.leaky_relu, UT.bn_act_train, UT.relu_up2_cat

    def bn_spy(h, module, slope=None):
        out = real_bn(h, module, slope)
        if slope is not None:
            seen.record(out[0])
        return out
    monkeypatch.setattr(arch.F, "leaky_relu", lambda h, s: (seen.record(h), real_leaky(h, s))[1])
    monkeypatch.setattr(UT, "bn_act_train", bn_spy)
    monkeypatch.setattr(UT, "relu_up2_cat", lambda a, b=None: (seen.record(ref.up_cat(a, b)), real_up(a, b))[1])
    with training.hip_routes_with_unet():
        out = net(x.to(DEV))
        names = graph_names(out)
        (out * G.to(DEV)).sum().backward()
    monkeypatch.undo()
    assert {"_BnActBackward", "_ReluUp2CatBackward"} <= names and len(seen.masks) == 15
    if filters == 32:
        assert {"_Conv3x3TrainBackward", "_ConvThinOutTrainBackward"} <= names

    def twin(dtype):
        t = copy.deepcopy(host).to(dtype)
        seen.at = seen.differ = seen.total = 0
        o = ref.twin_forward(t, x.to(dtype), seen)
        (o * G.to(dtype)).sum().backward()
        return t, o.detach()
    t64, o64 = twin(torch.float64)
    print(f"Unet({filters}): {seen.differ} of {seen.total} decisions differ from the fp64 twin's own signs")
    t32, o32 = twin(torch.float32)
    bound, _ = ref.grad_bound(o32, o64)
    worst = ref.check(f"Unet({filters}) output", out.detach(), o64, bound)
    g64, g32 = dict(t64.named_parameters()), dict(t32.named_parameters())
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        bound, _ = ref.grad_bound(g32[k].grad, g64[k].grad)
        worst = max(worst, ref.check(f"Unet({filters}) grad {k}", p.grad, g64[k].grad, bound))
    # the running statistics: a norm's input carries the fp32 error of the layers in front of it, which the operator's bound (one call's
    # roundings, test_bn_running_statistics_after_one_and_two_calls) does not cover: the gradient rule, E32 the fp32 twin's error
    b64, b32 = dict(t64.named_buffers()), dict(t32.named_buffers())
    for k, v in net.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(b64[k]) == 1
        elif "running" in k:
            bound, _ = ref.grad_bound(b32[k], b64[k])
            worst = max(worst, ref.check(f"Unet({filters}) {k}", v, b64[k], bound))
    print(f"Unet({filters}): largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_ten_adam_steps_lower_an_l1_depth_loss():
    net = make_unet(4, seed=2).to(DEV)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 256, 256, generator=gen).to(DEV)
    target = torch.rand(2, 3, 256, 256, generator=gen).to(DEV)
    optim = torch.optim.Adam(net.parameters(), lr=1e-3)
    history = []
    with training.hip_routes_with_unet():
        for _ in range(10):
            optim.zero_grad(set_to_none=True)
            loss = F.l1_loss(torch.sigmoid(net(x)), target)
            loss.backward()
            optim.step()
            history.append(float(loss.detach()))
    print(f"ten Adam steps, L1: {history[0]:.6f} -> {history[-1]:.6f}")
    assert all(h == h for h in history) and history[-1] < history[0]


def test_one_whole_step_against_the_spectral_routes():
    def step(context):
        opt = U.train_opts()
        torch.manual_seed(0)
        trainer = BaseModel(U.make_model(opt), opt).to(DEV)
        batch = U.make_batch(1, DEV, with_depth=False)
        torch.manual_seed(5)
        with context():
            losses, _ = trainer(batch)
        return {k: float(v.detach()) for k, v in losses.items() if torch.is_tensor(v) and v.numel() == 1}
    want, got = step(training.hip_routes_with_spectral), step(training.hip_routes_with_unet)
    assert set(want) == set(got) and "Total Loss" in got
    for k in want:
        rel = abs(got[k] - want[k]) / max(abs(want[k]), 1e-30)
        print(f"whole step {k}: {got[k]:.7g} against {want[k]:.7g}, relative {rel:.2e}")
        assert got[k] == got[k] and abs(got[k]) != float("inf") and rel <= 1e-4, k
