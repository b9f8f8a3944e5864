"""GPU: the training quantiser (csrc/vq_train.hip behind include/pixelsynth_vq_train.h, Quantize.forward in train() mode and its autograd
Function in vqvae2/vqvae.py, vqvae2/train.train_step).

Operator level: every output, statistic and buffer against the fp64 formulas of tests/_vq_train_ref.py on the kernel's own codes, inside
the DERIVED rounding bounds of that module (its docstring says where they come from).  Module level: modes, versions, gradients.  Network
level: a VQVAETop of the reference's sizes on two 64 x 64 images -- the tensors entering and leaving both quantisers inside the operator
bounds, twenty training steps, and the inference path seeing the tuned codebook.
"""
import pytest
import torch

import _vq_train_ref as ref
from pixelsynth_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}         # output -> the largest error / bound seen (printed by each check: the README's figures)


def _quantizer(D, K, seed=0):
    from pixelsynth_amd.vqvae2.vqvae import Quantize
    torch.manual_seed(seed)
    return Quantize(D, K).to(DEV).train()


def _state(q):
    return {k: v.detach().clone() for k, v in q.state_dict().items()}


def _latents(N, D, seed=1):
    return torch.randn(N, D, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _stats(z, idx, K):
    """The statistics kernel alone -> (counts, sums)"""
    N, D = z.shape
    need = _lib.call("ps_vq_train_workspace_bytes", N, D, K)
    ws = torch.empty(need, dtype=torch.uint8, device=z.device)
    counts, sums = torch.empty(K, dtype=torch.int32, device=z.device), torch.empty(D, K, device=z.device)
    _lib.call("ps_vq_train_stats_f32", z.contiguous(), idx.to(torch.int32).contiguous(), N, D, K, counts, sums, ws, need)
    return counts, sums


def _check_forward(name, q, z, before, out, arg_min=True):
    """One training forward of q on z (N, D) from the state `before`, its outputs `out`, against the fp64 formulas -> the expected values"""
    quantize, diff, ind = out
    N, D = z.shape
    K = q.n_embed
    assert quantize.shape == z.shape and quantize.dtype == torch.float32 and diff.shape == () and diff.dtype == torch.float32
    assert ind.shape == z.shape[:-1] and ind.dtype == torch.int64 and int(ind.min()) >= 0 and int(ind.max()) < K
    idx = ind.reshape(-1)
    exp = ref.expected(z, before["embed"], idx, before["cluster_size"], before["embed_avg"], q.decay, q.eps)
    if arg_min and N * K <= 1 << 20:        # the codes are a minimiser of the distance (ps_vq_nearest_f32's own tests pin the tie rule)
        dist = torch.cdist(z.cpu().double(), before["embed"].cpu().double().t()) ** 2
        assert (dist.gather(1, idx.cpu()[:, None])[:, 0] <= dist.min(1).values + 1e-5 * (1 + dist.min(1).values)).all()
    zc, ec = z.cpu(), before["embed"].cpu()
    e = ref.gather(ec, idx.cpu())
    assert torch.equal(quantize.cpu(), zc + (e - zc)), f"{name}: quantize is not torch's fp32 z + (e - z) bit for bit"
    b = exp["bound"]
    ref.check(f"{name} diff", diff, exp["diff"], b["diff"], WORST)
    counts, sums = _stats(z, idx, K)
    assert torch.equal(counts.cpu().long(), exp["counts"]), f"{name}: counts"
    ref.check(f"{name} sums", sums, exp["sums"], b["sums"], WORST)
    after = _state(q)
    for key in ("cluster_size", "embed_avg", "embed"):
        ref.check(f"{name} {key}", after[key], exp[key], b[key], WORST)
    return exp


def _update(name, q, z, **kw):
    before = _state(q)
    out = q(z)
    torch.cuda.synchronize()
    return _check_forward(name, q, z, before, out, **kw), out


# ------------------------------------------------------------------------------------------------------------------ operator level
def test_case_1_reference_sizes_odd_rows_two_updates():
    q = _quantizer(64, 512)
    assert not q.cluster_size.any()
    _update("N1003 D64 K512 first update", q, _latents(1003, 64, 1))
    _update("N1003 D64 K512 second update", q, _latents(1003, 64, 2))


def test_case_2_rows_no_multiple_of_4_channels_and_codes_padded():
    q = _quantizer(5, 37)
    exp, _ = _update("N131 D5 K37", q, _latents(131, 5, 3))
    assert int(exp["counts"].sum()) == 131
    _update("N131 D5 K37 second update", q, _latents(131, 5, 4))


def test_case_3_one_row():
    for D, K in ((64, 512), (5, 37)):
        q = _quantizer(D, K)
        exp, _ = _update(f"N1 D{D} K{K}", q, _latents(1, D, 5))
        assert int(exp["counts"].sum()) == 1 and int(exp["counts"].max()) == 1


def test_case_4_codebook_collapse_across_a_part_boundary():
    N, D, K = 2 * ref.PART_ROWS + 3, 64, 512
    assert ref.part_rows(N) == ref.PART_ROWS                      # three parts: one code owns rows on both sides of two boundaries
    q = _quantizer(D, K)
    with torch.no_grad():
        q.cluster_size.copy_(torch.rand(K, generator=torch.Generator().manual_seed(6)) + 0.5)
    before = _state(q)
    z = _latents(1, D, 7).expand(N, D).contiguous()
    exp, (_, _, ind) = _update("collapse", q, z)
    owner = int(ind[0])
    assert (ind == owner).all() and int(exp["counts"][owner]) == N and int(exp["counts"].sum()) == N
    counts, sums = _stats(z, ind.reshape(-1), K)
    dead = torch.arange(K, device=DEV) != owner
    assert not counts[dead].any() and not sums[:, dead].any()
    # dead codes: cluster_size = decay * old (one product in fp32), a finite codebook entry
    want = torch.tensor(q.decay, dtype=torch.float32, device=DEV) * before["cluster_size"]
    assert torch.equal(q.cluster_size[dead], want[dead])
    assert torch.isfinite(q.embed).all() and torch.isfinite(q.embed_avg).all()
    # ... and from an empty history: a dead code's size stays 0, its entry finite
    q0 = _quantizer(D, K)
    _update("collapse from zero", q0, z)
    assert not q0.cluster_size[dead].any() and float(q0.cluster_size[owner]) > 0 and torch.isfinite(q0.embed).all()


def test_case_5_the_reference_size_with_a_ragged_tail():
    N = 65536 + 37
    assert ref.part_rows(N) == 2 * ref.PART_ROWS
    q = _quantizer(64, 512)
    _update("N65573 D64 K512", q, _latents(N, 64, 8))


def test_case_6_two_identical_calls_give_the_same_bits():
    N = 2 * ref.PART_ROWS + 3
    z = _latents(N, 64, 9)
    runs = []
    for _ in range(2):
        q = _quantizer(64, 512, seed=3)
        zz = z.clone().requires_grad_()
        quantize, diff, ind = q(zz)
        g, = torch.autograd.grad((quantize, diff), zz, (torch.ones_like(quantize) * 0.25, torch.tensor(1.5, device=DEV)))
        counts, sums = _stats(z, ind.reshape(-1), 512)
        runs.append(dict(quantize=quantize.detach(), diff=diff.detach(), ind=ind, grad=g, counts=counts, sums=sums, **_state(q)))
    for key in runs[0]:
        assert torch.equal(runs[0][key], runs[1][key]), key


def test_case_7_the_movedim_view_gives_the_contiguous_copys_bits():
    feat = torch.randn(2, 64, 6, 5, generator=torch.Generator().manual_seed(10)).to(DEV)
    view = feat.movedim(1, -1)
    assert not view.is_contiguous()
    a, b = _quantizer(64, 512, seed=4), _quantizer(64, 512, seed=4)
    before = _state(a)
    got, want = a(view), b(view.contiguous())
    assert got[0].shape == (2, 6, 5, 64) and got[2].shape == (2, 6, 5)
    for p, r in zip(got, want):
        assert torch.equal(p, r)
    for key, v in _state(a).items():
        assert torch.equal(v, _state(b)[key]), key
    _check_forward("movedim view", a, view.reshape(-1, 64), before, (got[0].reshape(-1, 64), got[1], got[2].reshape(-1)))


# -------------------------------------------------------------------------------------------------------- modes and gradients
@pytest.mark.parametrize("N,D,K", [(1003, 64, 512), (131, 5, 37)])
def test_case_8_backward(N, D, K):
    q = _quantizer(D, K)
    before = _state(q)
    z = _latents(N, D, 11).requires_grad_()
    quantize, diff, ind = q(z)
    assert quantize.requires_grad and quantize.grad_fn is not None and diff.requires_grad and diff.grad_fn is not None
    assert not ind.requires_grad
    gen = torch.Generator().manual_seed(12)
    gq, gd = torch.randn(N, D, generator=gen).to(DEV), torch.tensor(-0.75, device=DEV)
    args = (z.detach().cpu().double(), before["embed"].cpu().double(), ind.cpu())     # e_n from the codebook BEFORE the update
    both, = torch.autograd.grad((quantize, diff), z, (gq, gd), retain_graph=True)
    want, term = ref.grad_input(*args, gq.cpu().double(), gd.cpu().double())
    ref.check(f"N{N} D{D} K{K} grad_input", both, want, ref.grad_bound(gq.cpu().double(), term), WORST)
    moved = ref.grad_input(z.detach().cpu().double(), q.embed.cpu().double(), ind.cpu(), gq.cpu().double(), gd.cpu().double())[0]
    assert ref.ratio(moved, want, ref.grad_bound(gq.cpu().double(), term)) > 1.0      # (the updated codebook would not pass)
    # grad_diff = 0, and no grad_diff at all: grad_quantize bit for bit
    zero, = torch.autograd.grad((quantize, diff), z, (gq, torch.zeros((), device=DEV)), retain_graph=True)
    assert torch.equal(zero, gq)
    alone, = torch.autograd.grad(quantize, z, gq, retain_graph=True)
    assert torch.equal(alone, gq)
    # only diff used downstream
    only, = torch.autograd.grad(diff * 3.0, z, retain_graph=True)
    want, term = ref.grad_input(*args, None, torch.tensor(3.0, dtype=torch.float64))
    ref.check(f"N{N} D{D} K{K} diff alone grad_input", only, want, ref.grad_bound(None, term), WORST)
    # a non-contiguous grad_quantize, through the views of the front end
    q2 = _quantizer(D, K)
    x = z.detach().reshape(1, N, D).requires_grad_()
    out = q2(x)[0]
    wide = torch.randn(1, N, 2 * D, generator=gen).to(DEV)
    sliced, = torch.autograd.grad(out, x, wide[..., ::2])
    assert torch.equal(sliced, wide[..., ::2])


def test_case_9_training_mode_under_no_grad_updates_the_buffers():
    a, b = _quantizer(64, 512, seed=5), _quantizer(64, 512, seed=5)
    z = _latents(300, 64, 13)
    before = _state(a)
    with torch.no_grad():
        out = a(z.clone().requires_grad_())
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    ref_out = b(z.clone().requires_grad_())
    for p, r in zip(out, ref_out):
        assert torch.equal(p, r.detach())
    after = _state(a)
    for key in after:
        assert torch.equal(after[key], _state(b)[key]) and not torch.equal(after[key], before[key]), key


def test_case_10_eval_mode_touches_nothing(monkeypatch):
    q = _quantizer(64, 512, seed=6).eval()
    before = _state(q)
    versions = [b._version for b in q.buffers()]
    z = _latents(300, 64, 14).reshape(3, 100, 64)
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (called.append(name), real(name, *a, **k))[1])
    quantize, diff, ind = q(z)
    assert called == ["ps_vq_nearest_f32"]
    assert ind.shape == (3, 100) and ind.dtype == torch.int64
    assert torch.equal(quantize, q.embed_code(ind)) and torch.equal(diff, (quantize - z).pow(2).mean())
    for key, v in _state(q).items():
        assert torch.equal(v, before[key]), key
    assert versions == [b._version for b in q.buffers()]
    # the same codes as the training route's
    del called[:]
    t_out = q.train()(z)
    assert torch.equal(t_out[2], ind) and any(n.startswith("ps_vq_train_") for n in called)


_NET = {}


def _net():
    """A VQVAETop of the reference's sizes on the device, two 64 x 64 images; built once"""
    if not _NET:
        from pixelsynth_amd.vqvae2.vqvae import VQVAETop
        torch.manual_seed(0)
        model = VQVAETop().to(DEV).train()
        gen = torch.Generator().manual_seed(15)
        coarse = torch.rand(2, 3, 8, 8, generator=gen) * 2 - 1
        img = torch.nn.functional.interpolate(coarse, size=(64, 64), mode="bilinear", align_corners=False).to(DEV)
        _NET.update(model=model, img=img)
    return _NET["model"], _NET["img"]


def test_case_11_an_update_moves_the_version_and_the_fast_path_key():
    from pixelsynth_amd.vqvae2.vqvae import _FastPath
    model, _ = _net()
    q = model.quantize_t
    key, versions = _FastPath.key_of(model), [b._version for b in (q.embed, q.cluster_size, q.embed_avg)]
    q(_latents(77, 64, 16))
    assert all(b._version > v for b, v in zip((q.embed, q.cluster_size, q.embed_avg), versions))
    assert _FastPath.key_of(model) != key


# ------------------------------------------------------------------------------------------------------------------ network level
def test_case_12_both_quantisers_inside_the_network():
    model, img = _net()
    seen = {}

    def watch(name, module):
        def pre(mod, args):
            z = args[0]
            seen[name] = dict(z=z.detach().clone(), before=_state(mod))
            z.register_hook(lambda g: seen[name].__setitem__("grad_input", g.detach().clone()))

        def post(mod, args, out):
            seen[name]["out"] = tuple(t.detach().clone() for t in out)
            out[0].register_hook(lambda g: seen[name].__setitem__("grad_quantize", g.detach().clone()))
            out[1].register_hook(lambda g: seen[name].__setitem__("grad_diff", g.detach().clone()))
            seen[name]["after"] = _state(mod)
        return [module.register_forward_pre_hook(pre), module.register_forward_hook(post)]

    handles = watch("top", model.quantize_t) + watch("bottom", model.quantize_b)
    try:
        model.zero_grad()
        out, latent = model(img)
        assert out.shape == img.shape and latent.shape == (1,)
        (torch.nn.functional.mse_loss(out, img) + 0.25 * latent.mean()).backward()
        torch.cuda.synchronize()
    finally:
        for h in handles:
            h.remove()
    for name, module, hw in (("top", model.quantize_t, 8), ("bottom", model.quantize_b, 16)):
        s = seen[name]
        assert s["z"].shape == (2, hw, hw, 64) and not s["z"].is_contiguous()
        z = s["z"].reshape(-1, 64)
        quantize, diff, ind = s["out"]
        idx = ind.reshape(-1)
        exp = ref.expected(z, s["before"]["embed"], idx, s["before"]["cluster_size"], s["before"]["embed_avg"], module.decay, module.eps)
        zc = z.cpu()
        assert torch.equal(quantize.reshape(-1, 64).cpu(), zc + (ref.gather(s["before"]["embed"].cpu(), idx.cpu()) - zc))
        ref.check(f"network {name} diff", diff, exp["diff"], exp["bound"]["diff"], WORST)
        for key in ("cluster_size", "embed_avg", "embed"):
            ref.check(f"network {name} {key}", s["after"][key], exp[key], exp["bound"][key], WORST)
        # (the bottom level's quantised latents are not decoded in forward: no grad_quantize reaches it, which counts as zero)
        assert ("grad_quantize" in s) == (name == "top") and "grad_diff" in s
        gq = s["grad_quantize"].reshape(-1, 64).cpu().double() if name == "top" else None
        gd = s["grad_diff"].reshape(()).cpu().double()
        want, term = ref.grad_input(zc.double(), s["before"]["embed"].cpu().double(), idx.cpu(), gq, gd)
        ref.check(f"network {name} grad_input", s["grad_input"].reshape(-1, 64), want, ref.grad_bound(gq, term), WORST)
    for pname, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, pname


def test_case_13_and_14_twenty_steps_and_the_inference_path_sees_them():
    from pixelsynth_amd.networks.f16x3 import decoder_conv
    from pixelsynth_amd.vqvae2.train import train_step
    import copy
    model, img = _net()
    untrained = copy.deepcopy(model).eval()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)            # the reference's learning rate
    losses = [train_step(model, opt, img) for _ in range(20)]
    print("reconstruction loss %.5f -> %.5f, latent loss %.5f -> %.5f over twenty steps" % (losses[0][0], losses[-1][0], losses[0][1], losses[-1][1]))
    assert all(isinstance(v, float) for pair in losses for v in pair)
    assert losses[-1][0] < losses[0][0]
    assert float(model.quantize_t.cluster_size.sum()) > 0 and float(model.quantize_b.cluster_size.sum()) > 0
    model.eval()
    # fixed codes among those in use: an entry nobody ever chose is the reference's embed_avg / (a size of about eps), of the order of 1e5
    alive = torch.nonzero(model.quantize_t.cluster_size > 1e-3)[:, 0]
    assert len(alive) >= 8
    codes = alive[torch.randint(0, len(alive), (1, 16, 16), generator=torch.Generator().manual_seed(17)).to(DEV)]
    start, tuned = untrained.decode_code(codes), model.decode_code(codes)
    with torch.no_grad():
        assert model._fast(codes, 128, 128) is not None            # (the hand-written route is the one under test)
    assert not torch.equal(tuned, start) and float((tuned - start).abs().max()) > 1e-3
    with decoder_conv("fp32"):
        want = model.decode_code(codes)
    torch.testing.assert_close(tuned, want, rtol=1e-3, atol=1e-4)
    # the codebook alone, too: one more update with the optimiser idle changes what the same codes decode to
    model.train()
    with torch.no_grad():
        model(img)
    model.eval()
    again = model.decode_code(codes)
    assert not torch.equal(again, tuned)
    with decoder_conv("fp32"):
        torch.testing.assert_close(again, model.decode_code(codes), rtol=1e-3, atol=1e-4)
    model.train()
