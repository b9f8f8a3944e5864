"""GPU: the plans and forms of csrc/disc_conv.hip and csrc/gan_train.hip that tests/test_disc_conv_gpu.py and tests/test_gan_train_gpu.py
never take, on the route cases of tests/_disc_conv_ref.py and tests/_gan_train_ref.py (tests/test_disc_routes_cpu.py asserts, without a
GPU, that every case reaches its branch and that no shape of the operator tests does).  Every case goes through the operator tests' own
bodies -- their checks and bounds unchanged: rules 1 and 2 of _disc_conv_ref.check, stat_bounds, y_bound, grad_bound and feat_value_bound
of _gan_train_ref -- and the named ones through the C ABI as well, with every output NaN-filled inside rims of sentinel floats and the
workspace at exactly its stated size, every byte 0xff, inside rims of its own (tests/_rims.py): an element left unwritten, a store
outside an output and a slab read before it was written all show.  Every reference is torch fp64 on the host.  docs/LAB_NOTEBOOK.md
section 19 has the table per case."""
import ctypes
import re

import pytest
import torch

import _disc_conv_ref as ref
import _gan_train_ref as gref
import test_disc_conv_gpu as conv_ops
import test_gan_train_gpu as gan_ops
from _rims import DEV, guarded, guarded_bytes, untouched, untouched_bytes
from pixelsynth_amd import _lib
from pixelsynth_amd.networks import disc_conv as DC, f16x3, gan_train as GT
from test_disc_conv_gpu import _clear, _flags, _run

pytestmark = pytest.mark.gpu
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


# ---------------------------------------------------------------- 1. the convolution's route cases through the operator tests' bodies
@pytest.mark.parametrize("shape", ref.ROUTE_SHAPES, ids=_ids)
def test_integers_bit_for_bit_on_a_route(shape):
    assert _lib.call("ps_disc_conv_parts", *shape, 2) == ref.plan(*shape).parts
    conv_ops.integers_bit_for_bit(shape)


@pytest.mark.parametrize("shape", ref.ROUTE_SHAPES, ids=_ids)
def test_accuracy_under_both_rules_on_a_route(shape):
    conv_ops.accuracy_under_both_rules(shape)


# ---------------------------------------------------------------- 2. through the C ABI with rims
class _Abi:
    """Both entry points on host operands: y, grad_x, grad_weight and scale2 NaN-filled inside rims, the workspace of exactly
    ps_disc_conv_workspace_bytes bytes (less `short`), 0xff-filled and 256-byte aligned, inside rims"""

    def __init__(self, x, w, g, stride, need=(True, True), short=0):
        B, Ci, H, W = x.shape
        Co = w.size(0)
        self.sizes = (B, Ci, Co, H, W, stride, 2)
        self.need = _lib.call("ps_disc_conv_workspace_bytes", *self.sizes)
        assert self.need == ref.workspace_bytes(*self.sizes)[0]
        self.x, self.w, self.g = x.to(DEV), w.to(DEV), g.to(DEV)
        self.n = dict(y=g.numel(), gx=x.numel() if need[0] else 0, gw=w.numel() if need[1] else 0, scale2=2)
        self.bufs = {k: guarded(n) for k, n in self.n.items() if n}
        self.nbytes = self.need - short
        self.wbuf, self.ws, self.at = guarded_bytes(self.nbytes)
        self.flag, self.grad_flag = f16x3.flag(torch.device(DEV)), f16x3.grad_flag(torch.device(DEV))

    def out(self, k):
        return self.bufs[k][1] if k in self.bufs else None

    def forward(self):
        _lib.call("ps_disc_conv_forward_f16x3", self.x, self.w, *self.sizes, self.out("y"), self.flag, self.ws, self.nbytes)

    def backward(self):
        _lib.call("ps_disc_conv_backward_f16x3", self.x, self.w, self.g, *self.sizes, self.out("gx"), self.out("gw"), self.out("scale2"),
                  self.flag, self.grad_flag, self.ws, self.nbytes)

    def rims_intact(self):
        torch.cuda.synchronize()
        return all(untouched(buf, self.n[k]) for k, (buf, _) in self.bufs.items()) and untouched_bytes(self.wbuf, self.at, self.nbytes)

    def written(self, *names):
        return all(not torch.isnan(self.out(k)).any() for k in names if k in self.bufs)

    def nothing_written(self):
        return all(torch.isnan(o).all() for _, o in self.bufs.values()) and bool((self.ws == 255).all())


def _abi_run(x, w, g, stride, need=(True, True)):
    """_run of tests/test_disc_conv_gpu.py through the entry points themselves: every output written everywhere, every rim intact after
    both passes"""
    a = _Abi(x, w, g, stride, need)
    a.forward()
    assert a.rims_intact() and a.written("y") and torch.isnan(a.out("scale2")).all()
    a.backward()
    assert a.rims_intact() and a.written("y", "gx", "gw", "scale2")
    _abi_run.scale2 = a.out("scale2").tolist()
    shape = lambda k, like: a.out(k).clone().view(like.shape) if k in a.bufs else None  # noqa: E731
    return shape("y", g), shape("gx", x), shape("gw", w)


@pytest.mark.parametrize("shape", ref.ABI_SHAPES, ids=_ids)
def test_through_the_abi_inside_rims(shape):
    conv_ops.integers_bit_for_bit(shape, run=_abi_run)
    assert _abi_run.scale2 == [2.0 ** 13, 2.0 ** -13]                          # (max |g| = 3: the scale came back through its rim)
    conv_ops.accuracy_under_both_rules(shape, run=_abi_run)
    # one byte fewer of workspace is refused by both passes, with both sizes in the message, and nothing is touched
    x, w, g = ref.integers(shape)[:3]
    a = _Abi(x, w, g, shape[5], short=1)
    _clear()
    for call in (a.forward, a.backward):
        with pytest.raises(RuntimeError) as err:
            call()
        assert re.search(rf"workspace of {a.need - 1} bytes, {a.need} needed", str(err.value)), str(err.value)
        assert a.rims_intact() and a.nothing_written() and _flags() == (0, 0)


# ---------------------------------------------------------------- 3. a tiny gradient under the held exponent
@pytest.mark.parametrize("run", [_run, _abi_run], ids=["function", "abi"])
def test_a_tiny_gradient_under_the_held_exponent(run):
    """max |g| = 3 x 2^-115 asks for a scale of 2^128, which is no fp32: k_disc_conv_amax_finish holds the exponent at 126.  x 2^8 and
    w 2^16 keep every gradient a normal fp32, so the results are the fp64 ones bit for bit (the body asserts both flags clear)"""
    operands = ref.scaled_integers(ref.TINY_SHAPE, *ref.TINY_EXPONENTS)
    assert operands[2].abs().max().item() == 3 * 2.0 ** -115
    conv_ops.integers_bit_for_bit(ref.TINY_SHAPE, run=run, operands=operands)
    scale2 = DC._DiscConv.last_scale2.tolist() if run is _run else _abi_run.scale2
    assert scale2 == [2.0 ** 126, 2.0 ** -126], scale2


# ---------------------------------------------------------------- 4. the weight's words
WORDS_SHAPE = (2, 64, 64, 9, 11, 2)          # test_overflow_words' own


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_weight_that_is_not_finite_raises_its_words(bad):
    """The header's last paragraph: a scaled weight that is not finite raises *overflow in the forward pass and *grad_overflow in the
    backward pass, where grad_x packs it again; grad_weight alone does not meet the weight"""
    x, w, g = ref.inputs(WORDS_SHAPE, seed=4)
    wb = w.clone()
    wb[5, 3, 2, 1] = bad
    for need, after in (((True, True), (0, 1)), ((True, False), (0, 1)), ((False, True), (0, 0))):
        xd, wd = x.to(DEV).requires_grad_(need[0]), wb.to(DEV).requires_grad_(need[1])
        _clear()
        y = DC.conv4x4_train(xd, wd, WORDS_SHAPE[5])
        assert _flags() == (1, 0), (bad, need)                     # the forward raises `flag` alone
        _clear()
        y.backward(g.to(DEV))                                      # a clean g and a clean x
        assert _flags() == after, (bad, need)
        if need == (False, True):                                  # ... and the weight gradient is the clean weight's
            _clear()
            assert torch.equal(wd.grad, _run(x, w, g, WORDS_SHAPE[5], need=need)[2]) and _flags() == (0, 0)
    _clear()


def test_a_weight_of_zeros():
    """max |w| = 0: sw = 1, y and grad_x are +0 everywhere, grad_weight is the usual one, no word rises"""
    x, w, g, _, _, gw64 = ref.integers(WORDS_SHAPE)
    _clear()
    for run in (_run, _abi_run):
        y, gx, gw = run(x, torch.zeros_like(w), g, WORDS_SHAPE[5])
        assert not y.view(torch.int32).any() and not gx.view(torch.int32).any()            # the bits: +0
        assert torch.equal(gw.cpu(), gw64) and _flags() == (0, 0)
    assert torch.equal(gw, _run(x, w, g, WORDS_SHAPE[5])[2])


# ---------------------------------------------------------------- 5. the norm's forms
def _norm_inside_rims(x, dy=None):
    """_norm of tests/test_gan_train_gpu.py with y, mean, rstd and dx NaN-filled inside rims: every value written, every rim intact"""
    xd = x.to(DEV).contiguous()
    planes, hw = xd.size(0) * xd.size(1), xd.size(2) * xd.size(3)
    n = dict(y=xd.numel(), mean=planes, rstd=planes, dx=xd.numel() if dy is not None else 0)
    bufs = {k: guarded(v) for k, v in n.items() if v}
    o = {k: b[1] for k, b in bufs.items()}
    _lib.call("ps_in_lrelu_forward_f32", xd, planes, hw, gan_ops.EPS, gan_ops.SLOPE, o["y"], o["mean"], o["rstd"], None, 0)
    if dy is not None:
        _lib.call("ps_in_lrelu_backward_f32", xd, dy.to(DEV).contiguous(), o["mean"], o["rstd"], planes, hw, gan_ops.SLOPE, o["dx"], None, 0)
    torch.cuda.synchronize()
    assert all(not torch.isnan(v).any() for v in o.values()), [k for k, v in o.items() if torch.isnan(v).any()]
    assert all(untouched(buf, n[k]) for k, (buf, _) in bufs.items()), [k for k, (buf, _) in bufs.items() if not untouched(buf, n[k])]
    out = [o["y"].view(xd.shape), o["mean"].view(xd.shape[:2]), o["rstd"].view(xd.shape[:2])] + ([o["dx"].view(xd.shape)] if dy is not None else [])
    return [t.cpu() for t in out]


@pytest.mark.parametrize("shape", gref.NORM_ROUTE_CASES, ids=_ids)
def test_norm_forms_against_fp64(shape):
    print("form:", gref.form(shape[3]))
    gan_ops.norm_against_fp64(shape, norm=_norm_inside_rims)


# ---------------------------------------------------------------- 6. staged feature matching
@pytest.mark.parametrize("name", list(gref.FEAT_ROUTE_LISTS))
def test_staged_feature_matching(name):
    shapes = gref.FEAT_ROUTE_LISTS[name]
    maps, per_map, total = gan_ops.feature_matching_against_fp64(name, shapes)
    # the entry points themselves: per_map, total and every gradient inside rims, the workspace at exactly its stated size inside rims
    w, gt, n = 5.0, 0.75, len(maps)
    dev = [m.to(DEV) for m in maps]
    ptrs, halves, weights = GT._tables(dev, w)
    need = _lib.call("ps_gan_feat_workspace_bytes", halves, n)
    assert need == -(-8 * sum(gref.feat_tiles(shapes)) // 256) * 256
    wbuf, ws, at = guarded_bytes(need)
    pbuf, pm = guarded(n)
    tbuf, tot = guarded(1)
    _lib.call("ps_gan_feat_l1_f32", ptrs, halves, weights, n, pm, tot, ws, need)
    grads = [guarded(m.numel()) for m in maps]
    gptrs = (ctypes.c_void_p * n)(*[g.data_ptr() for _, g in grads])
    _lib.call("ps_gan_feat_l1_backward_f32", ptrs, halves, weights, n, torch.tensor([gt], device=DEV), gptrs)
    torch.cuda.synchronize()
    assert untouched(pbuf, n) and untouched(tbuf, 1) and untouched_bytes(wbuf, at, need)
    assert torch.equal(pm.cpu(), per_map) and torch.equal(tot.cpu(), total)                     # the Function's bits, under the bound there
    for (gbuf, got), want, m in zip(grads, gref.feat_backward32(maps, [w] * n, gt), maps):
        assert untouched(gbuf, m.numel()) and not torch.isnan(got).any()
        assert torch.equal(gan_ops._int_bits(got.cpu().view(m.shape)), gan_ops._int_bits(want))
