"""CPU-only: the host side of the training quantiser (csrc/vq_train.hip, vqvae2/vqvae.py, distributed.sum_over_ranks): the C ABI of
libpixelsynth_vq_train.so against its header and bindings, its refusals before anything is launched, the fp64 formulas and bounds of
tests/_vq_train_ref.py against torch autograd and an independent restatement, the front end's refusal of CPU tensors, and the sum of
the statistics over two gloo ranks."""
import os
import re
import socket
import subprocess
import sys

import pytest
import torch

import _vq_train_ref as ref
from abi_util import ROOT, assert_library_matches_header
from pixelsynth_amd import _lib, _libraries


def test_the_registry_has_the_vq_train_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "vq_train")
    assert entry.so == "libpixelsynth_vq_train.so" and entry.headers == ("pixelsynth_vq_train.h",)
    assert entry.last_error == "ps_vq_train_last_error"
    assert [u for u, _ in entry.units] == ["vq_train.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("vq_train")
    assert set(protos) == set(_lib.VQ_TRAIN_PROTOS) == {
        "ps_vq_train_last_error", "ps_vq_train_workspace_bytes", "ps_vq_train_stats_f32", "ps_vq_train_quantize_f32",
        "ps_vq_train_update_f32", "ps_vq_train_backward_f32"}
    # the constants the tests' split and bounds are made of are the header's
    header = open(os.path.join(ROOT, "include", "pixelsynth_vq_train.h")).read()
    assert int(re.search(r"#define PS_VQ_TRAIN_MAX_PARTS (\d+)", header).group(1)) == ref.MAX_PARTS
    assert int(re.search(r"#define PS_VQ_TRAIN_PART_ROWS (\d+)", header).group(1)) == ref.PART_ROWS
    # the pinned library does not export what this one adds
    assert not any(hasattr(_lib.lib(), fn) for fn in protos)


def test_workspace_bytes():
    ws = _lib.library("vq_train").ps_vq_train_workspace_bytes
    for args in ((0, 64, 512), (-1, 64, 512), (100, 0, 512), (100, 65, 512), (100, 64, 0), (100, 64, -5), ((1 << 30) + 1, 64, 512),
                 (100, 64, (1 << 20) + 1)):
        assert ws(*args) == 0, args
    pad = lambda v: -(-v // 16) * 16
    for N, D, K in ((1, 1, 1), (131, 5, 37), (1003, 64, 512), (65536 + 37, 64, 512), (262144, 64, 512), (3 * ref.PART_ROWS * ref.MAX_PARTS + 1, 64, 512)):
        rows = ref.part_rows(N)
        parts = -(-N // rows)
        assert rows % ref.PART_ROWS == 0 and 1 <= parts <= ref.MAX_PARTS and (parts - 1) * rows < N
        assert rows == ref.PART_ROWS or -(-N // (rows - ref.PART_ROWS)) > ref.MAX_PARTS       # (the smallest such multiple)
        # one padded table of sums and one of counts per part, one fp64 partial per 16384 elements, K floats of s; four aligned regions
        least = parts * pad(D) * pad(K) * 4 + parts * pad(K) * 4 + -(-N * D // 16384) * 8 + K * 4
        got = ws(N, D, K)
        assert least <= got <= least + 4 * 256 and got % 256 == 0, (N, D, K, got, least)
    assert ws(262144, 64, 512) <= ref.MAX_PARTS * 64 * 512 * 4 + (1 << 20)


def test_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("vq_train")
    err = L.ps_vq_train_last_error
    p = torch.zeros(64).data_ptr()                     # (any aligned non-null address: the arguments are refused before it is looked at)
    N, D, K = 131, 5, 37
    need = L.ps_vq_train_workspace_bytes(N, D, K)
    assert need > 0

    def calls(fn, names, ok):
        def bad(**kw):
            assert set(kw) <= set(names), kw
            return fn(*[kw.get(n, v) for n, v in zip(names, ok)], None)
        return bad

    stats = calls(L.ps_vq_train_stats_f32, ["z", "idx", "N", "D", "K", "counts", "sums", "ws", "bytes"], [p, p, N, D, K, p, p, p, need])
    quant = calls(L.ps_vq_train_quantize_f32, ["z", "idx", "rows", "N", "D", "K", "q", "diff", "ws", "bytes"],
                  [p, p, p, N, D, K, p, p, p, need])
    upd = calls(L.ps_vq_train_update_f32, ["counts", "sums", "D", "K", "decay", "alpha", "eps", "cs", "avg", "embed", "ws", "bytes"],
                [p, p + 64, D, K, 0.99, 0.01, 1e-5, p, p, p + 128, p, need])
    bwd = calls(L.ps_vq_train_backward_f32, ["z", "idx", "rows", "gq", "gd", "N", "D", "K", "gi"], [p, p, p, p, p, N, D, K, p])
    for name, fn, pointers, sized in (("stats", stats, ("z", "idx", "counts", "sums"), True), ("quantize", quant, ("z", "idx", "rows", "q", "diff"), True),
                                      ("update", upd, ("counts", "sums", "cs", "avg", "embed"), False), ("backward", bwd, ("gi",), True)):
        tag = f"vq_train_{name}".encode()
        for ptr_name in pointers:
            assert fn(**{ptr_name: None}) != 0 and b"null pointer" in err() and tag in err(), (name, ptr_name)
        for size in ("N", "D", "K") if sized else ("D", "K"):
            for v in (0, -3):
                assert fn(**{size: v}) != 0 and f"{size} = {v}".encode() in err() and tag in err(), (name, size, v)
        assert fn(D=65) != 0 and b"D = 65, more than 64" in err() and b"ps_vq_nearest_f32" in err()
        assert fn(K=(1 << 20) + 1) != 0 and b"2^20 codes" in err()
        if name != "backward":
            assert fn(ws=None) != 0 and b"null pointer (workspace)" in err()
            assert fn(bytes=0) != 0 and b"workspace of 0 bytes" in err()
            assert fn(ws=p + 4) != 0 and b"aligned to 16 bytes" in err()
    assert stats(N=(1 << 30) + 1) != 0 and b"2^30 vectors" in err()
    assert stats(bytes=need - 1) != 0 and b"workspace of" in err() and str(need).encode() in err()
    assert quant(bytes=need - 1) != 0 and b"workspace of" in err() and str(need).encode() in err()
    small = L.ps_vq_train_workspace_bytes(1, D, K)
    assert upd(bytes=small - 1) != 0 and b"workspace of" in err() and str(small).encode() in err()
    assert upd(embed=p) != 0 and b"embed_out cannot be" in err()
    # backward: either gradient may be missing, not both; the commitment term needs z, idx and the codebook
    assert bwd(gq=None, gd=None) != 0 and b"both gradients" in err()
    for ptr_name in ("z", "idx", "rows"):
        assert bwd(**{ptr_name: None}) != 0 and b"grad_diff needs" in err()
    # through the binding: a CPU tensor is refused by name before a stream is looked up
    with pytest.raises(RuntimeError, match=r"ps_vq_train_backward_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_vq_train_backward_f32", torch.zeros(2, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(3, 2), torch.zeros(2, 2),
                  None, 2, 2, 3, torch.zeros(2, 2))


def _case(N, D, K, seed=0):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(N, D, generator=gen)
    embed = torch.randn(D, K, generator=gen)
    idx = torch.randint(0, K, (N,), generator=gen)
    return z, embed, idx


@pytest.mark.parametrize("N,D,K", [(7, 3, 4), (33, 5, 6)])
def test_the_fp64_formulas_against_autograd(N, D, K):
    z, embed, idx = _case(N, D, K)
    z64, e64 = z.double().requires_grad_(), embed.double()
    # gradcheck on the commitment term, a true function of z; the straight-through output is CONSTANT in z numerically (its value is
    # the code) and the identity by definition, so finite differences have nothing to say about it: autograd's rule is checked below
    assert torch.autograd.gradcheck(lambda t: ref.quantize(t, e64, idx)[1], (z64,))
    scale = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t, gd: ref.grad_input(t, e64, idx, None, gd)[0], (z64, scale))
    gen = torch.Generator().manual_seed(1)
    gq, gd = torch.randn(N, D, generator=gen, dtype=torch.float64), torch.randn((), generator=gen, dtype=torch.float64)
    q, diff = ref.quantize(z64, e64, idx)
    want, = torch.autograd.grad((q, diff), z64, (gq, gd), retain_graph=True)
    got, term = ref.grad_input(z64.detach(), e64, idx, gq, gd)
    assert (got - want).abs().max() <= 1e-14 * max(1.0, float(want.abs().max()))
    only_diff, = torch.autograd.grad(diff, z64, gd, retain_graph=True)
    assert (ref.grad_input(z64.detach(), e64, idx, None, gd)[0] - only_diff).abs().max() <= 1e-14
    assert torch.equal(ref.grad_input(z64.detach(), e64, idx, gq, None)[0], gq)
    # the value is the reference's: the selected codebook entry up to one rounding, and mean((e - z)^2)
    e = ref.gather(e64, idx)
    assert (q.detach() - e).abs().max() <= 1e-15 * 8 and abs(float(diff.detach()) - float(((e - z64.detach()) ** 2).mean())) <= 1e-15
    # the bound holds torch's own fp32 evaluation of the same formula, and a dropped commitment term does not pass it
    g32, _ = ref.grad_input(z, embed, idx, gq.float(), gd.float())
    w64, t64 = ref.grad_input(z.double(), embed.double(), idx, gq.float().double(), gd.float().double())
    bound = ref.grad_bound(gq.float().double(), t64)
    assert ref.check("torch fp32 grad_input", g32, w64, bound) <= 1.0
    assert ref.ratio(gq.float(), w64, bound) > 1.0


@pytest.mark.parametrize("N,D,K", [(7, 3, 4), (200, 5, 6)])
def test_the_statistics_and_the_update_against_the_one_hot_form(N, D, K):
    z, embed, idx = _case(N, D, K, seed=2)
    idx[idx == K - 1] = 0                                      # a code nobody chose
    counts, sums = ref.stats(z.double(), idx, K)
    c1, s1 = ref.stats_onehot(z.double(), idx, K)
    assert torch.equal(counts.double(), c1) and (sums - s1).abs().max() <= 1e-13 and int(counts.sum()) == N and counts[K - 1] == 0
    assert sums.shape == (D, K) and not sums[:, K - 1].any()
    decay, eps = 0.99, 1e-5
    gen = torch.Generator().manual_seed(4)
    cs, avg = torch.rand(K, generator=gen) * 3, torch.randn(D, K, generator=gen)
    exp = ref.expected(z, embed, idx, cs, avg, decay, eps)
    # the reference's own statement of the update, in fp64 with in-place operations
    cs2, avg2 = cs.double().clone(), avg.double().clone()
    cs2.mul_(decay).add_(c1, alpha=1 - decay)
    avg2.mul_(decay).add_(s1, alpha=1 - decay)
    n = cs2.sum()
    size = (cs2 + eps) / (n + K * eps) * n
    assert (exp["cluster_size"] - cs2).abs().max() <= 1e-14 and (exp["embed_avg"] - avg2).abs().max() <= 1e-13
    assert (exp["embed"] - avg2 / size.unsqueeze(0)).abs().max() <= 1e-12 * float((avg2 / size).abs().max())
    assert abs(float(exp["s"].sum() - n)) <= 1e-12 * float(n)   # (the smoothed sizes keep the total)
    # the bounds hold the same steps in torch fp32, and one dropped row does not pass them
    c32, s32 = ref.stats(z, idx, K)
    b = exp["bound"]
    assert ref.check("torch fp32 sums", s32, exp["sums"], b["sums"]) <= 1.0
    cs32 = cs.clone().mul_(decay).add_(c32.float(), alpha=1 - decay)
    avg32 = avg.clone().mul_(decay).add_(s32, alpha=1 - decay)
    n32 = cs32.sum()
    e32 = avg32 / ((cs32 + eps) / (n32 + K * eps) * n32).unsqueeze(0)
    assert ref.check("torch fp32 cluster_size", cs32, exp["cluster_size"], b["cluster_size"]) <= 1.0
    assert ref.check("torch fp32 embed_avg", avg32, exp["embed_avg"], b["embed_avg"]) <= 1.0
    assert ref.check("torch fp32 embed", e32, exp["embed"], b["embed"]) <= 1.0
    q32 = z + (ref.gather(embed, idx) - z)
    assert ref.check("torch fp32 diff", (q32 - z).pow(2).mean(), exp["diff"], b["diff"]) <= 1.0
    _, dropped = ref.stats(z[1:].double(), idx[1:], K)
    assert ref.ratio(dropped, exp["sums"], b["sums"]) > 1.0
    with pytest.raises(AssertionError, match="must be exact"):
        bad = exp["sums"].clone()
        bad[0, K - 1] = 1e-30
        ref.ratio(bad, exp["sums"], b["sums"])


def test_part_rows_is_a_function_of_n_alone():
    assert ref.part_rows(1) == ref.part_rows(ref.PART_ROWS * ref.MAX_PARTS) == ref.PART_ROWS
    assert ref.part_rows(ref.PART_ROWS * ref.MAX_PARTS + 1) == 2 * ref.PART_ROWS
    assert ref.part_rows(262144) == 262144 // ref.MAX_PARTS


def test_training_mode_refuses_a_cpu_tensor_by_name():
    from pixelsynth_amd.vqvae2.vqvae import Quantize, VQVAETop
    q = Quantize(4, 8)
    assert q.training
    with pytest.raises(RuntimeError, match=r"Quantize\.forward \(training mode\).*no CPU fallback"):
        q(torch.zeros(3, 4))
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"Quantize\.forward \(training mode\).*no CPU fallback"):
        q(torch.zeros(2, 3, 4))
    before = {k: v.clone() for k, v in q.state_dict().items()}
    assert all(torch.equal(v, before[k]) for k, v in q.state_dict().items())
    net = VQVAETop(channel=16, n_res_block=1, n_res_channel=8, embed_dim=4, n_embed=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 3, 16, 16))
    from pixelsynth_amd.vqvae2 import train
    assert callable(train.train_step)


def test_sum_over_ranks_single_process():
    from pixelsynth_amd import distributed as D
    assert not torch.distributed.is_initialized()
    a, b = torch.arange(4, dtype=torch.int32), torch.ones(2, 3)
    got = D.sum_over_ranks(a, b)
    assert got[0] is a and got[1] is b and a._version == 0 and b._version == 0
    assert torch.equal(a, torch.arange(4, dtype=torch.int32)) and torch.equal(b, torch.ones(2, 3))


def test_sum_over_ranks_across_ranks():
    """gloo, world size 2: each rank holds the statistics of half the rows, both end with the full sums."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "tests", "_sum_over_ranks_worker.py")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
