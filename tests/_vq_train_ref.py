"""The fp64 side of the tests of the training quantiser (csrc/vq_train.hip, vqvae2/vqvae.py: Quantize.forward in train() mode): the
expected outputs, statistics, EMA update and gradient on the CPU, and the rounding bounds.  Not a test module.

The codes are GIVEN (the kernel's own idx): a near-tie of the arg-min cannot enter a comparison, so no case is left out.

Expected values (z (N,D), embed (D,K), idx (N), all as the fp32 values they are, computed in fp64; decay, eps the module's Python floats,
alpha = 1 - decay in double):
    e_n = embed[:, idx[n]]            r = e_n - z_n            quantize = z + r            diff = mean(r^2)
    counts[k] = #{n: idx[n] = k}      sums[d][k] = sum_{n: idx[n] = k} z[n][d]
    cluster_size' = decay cluster_size + alpha counts          embed_avg' = decay embed_avg + alpha sums
    n = sum_k cluster_size'           s = (cluster_size' + eps) / (n + K eps) n            embed' = embed_avg' / s
    grad_input = grad_quantize + grad_diff 2 / (N D) (z - e_n)

THE BOUNDS are derived, not measured.  u = 2^-24 (half an ulp, relative); 1.01 pays for the second-order terms ((1 + u)^j - 1 <= 1.01 j u
for j u < 0.01).

counts      exact (integer adds).
sums        the terms enter the MFMA as z * 1 (exact) and z * 0 = 0 (exact), so a sum is fp32 additions of its m = counts[k] terms,
            split into <= MAX_PARTS chains that are added afterwards.  Any order of adding m terms rounds m - 1 times, each rounding at
            most u times a partial sum <= sum |terms|:  |d sums[d][k]| <= 1.01 m u sum_{n in k} |z[n][d]|.  A code nobody chose: exactly 0.
quantize    z + (e - z) in IEEE fp32 with contraction off: bit-identical to torch's fp32 `z + (e - z)` on the CPU.
diff        r is rounded once (relative u), so r^2 is off by 2u relatively; squares and sum are fp64 (2^-53 each, N D of them: nothing
            at 2^-24), the quotient is rounded to fp32 once (u):  |d diff| <= 4 u diff.
cluster_size, embed_avg
            new = fl(fl(decay_f old) + fl(alpha_f stat)): decay_f and alpha_f are the fp32 roundings of the doubles (u each), each
            product rounds once (u), the sum once (u, of at most the sum of the magnitudes):
            |d new| <= 1.01 (3 u (|decay old| + |alpha stat|) + alpha |d stat|),  |d stat| = 0 for counts (below 2^24) and the bound
            above for sums.
n           the fp64 sum of the fp32 cluster sizes, rounded to fp32: sum_k |d cluster_size'[k]| + u n <= 4.03 u n + ...: relative
            R_N = 1.01 * 4 u (every term is >= 0, so relative errors do not grow in the sum).
s           numerator cluster_size' + eps_f: 3 u (cluster size) , u (eps_f), u (the sum) of non-negative terms: <= 4 u relative
            (3 u of the larger share and u of the sum; eps_f's u applies to its own share, never more than the 3 u).  Denominator
            n + fl(K eps_f): 4 u (n) or 2 u (K eps_f) on the shares, u for the sum: 5 u.  Quotient u, times n (4 u) u:
            R_S = 1.01 * (4 + 5 + 1 + 4 + 1) u = 1.01 * 15 u relative.
embed       embed' = fl(embed_avg' / s): |d embed'| <= |d embed_avg'| / s + |embed_avg'| / s (R_S + 1.01 u), with the expected s and
            embed_avg' (second-order terms in the 1.01s).
grad_input  c = grad_diff 2 / (N D) is kept in fp64; z - e rounds once, the product once: the second term t = c (z - e) is off by at
            most 2 u |t| -- 3 u |t| allowed; the sum rounds once, u |grad_quantize + t| <= u (|grad_quantize| + |t|):
            |d grad_input| <= 1.01 u (|grad_quantize| + 4 |t|).  With grad_diff = 0: grad_quantize bit for bit.

A code outside 0 .. K-1 (the header's contract: a row of zeros in the gathers, no code in the statistics) is expected by the same formulas
on a codebook with a column of zeros appended and every such code sent to it: with_zero_row().
"""
from collections import namedtuple

import torch

U = 2.0 ** -24
MAX_PARTS = 128                    # = PS_VQ_TRAIN_MAX_PARTS  (test_vq_train_cpu.py reads the header)
PART_ROWS = 512                    # = PS_VQ_TRAIN_PART_ROWS
R_N = 1.01 * 4 * U
R_S = 1.01 * 15 * U


def part_rows(N):
    """Rows per part for N vectors (include/pixelsynth_vq_train.h): the smallest multiple of PART_ROWS that gives <= MAX_PARTS parts"""
    blocks = -(-N // PART_ROWS)
    return PART_ROWS * -(-blocks // MAX_PARTS)


TILE, CT, Q_ELEMS = 16, 2, 16384   # csrc/vq_train.hip's: channels / codes of an MFMA tile, code tiles a wave keeps, k_quantize's workgroup
VqPlan = namedtuple("VqPlan", "dt kt wpp part_rows parts qwgs bytes")


def plan(N, D, K):
    """csrc/vq_train.hip's make_plan: channel tiles (the DT of k_stats_parts<DT>), code tiles, waves per part, the split of the rows,
    k_quantize's workgroups, and the workspace's size (which tests/test_train_routes2_cpu.py holds to the library's own)"""
    up = lambda v: -(-v // 256) * 256
    Dp, Kp = -(-D // TILE) * TILE, -(-K // TILE) * TILE
    rows = part_rows(N)
    parts, qwgs = -(-N // rows), -(-N * D // Q_ELEMS)
    qpart = up(up(parts * Dp * Kp * 4) + parts * Kp * 4)
    return VqPlan(Dp // TILE, Kp // TILE, -(-Kp // TILE // CT), rows, parts, qwgs, up(up(qpart + qwgs * 8) + K * 4))


RouteCase = namedtuple("RouteCase", "id shape why")          # shape (N, D, K)
ROUTE_CASES = [
    RouteCase("dt3_parts3", (1027, 33, 40), "DT = 3 with one live channel in its last tile, an odd number of code tiles, three parts; "
                                            "k_quantize's second and third workgroup start off channel 0"),
    RouteCase("dt3_one_code_tile", (700, 48, 16), "DT = 3 on full tiles; K <= 16: one wave per part, c_hi never true"),
    RouteCase("dt2", (515, 20, 100), "DT = 2, seven code tiles on four waves, two parts"),
    RouteCase("dt2_edge", (1027, 17, 33), "DT = 2 with one live channel in the second tile; k_quantize's second workgroup starts at channel 13"),
    RouteCase("dt1_quantize_walk", (3300, 5, 37), "seven parts at DT = 1; the D = 5 walk of k_quantize across a workgroup boundary"),
]
# (N, D, K) of the operator tests of tests/test_vq_train_gpu.py
OPERATOR_SHAPES = [(1003, 64, 512), (131, 5, 37), (1, 64, 512), (1, 5, 37), (1027, 64, 512), (65573, 64, 512)]


def _f64(t):
    return t.detach().cpu().double()


def gather(embed, idx):
    """embed (D,K), idx (N) -> e (N,D)"""
    return embed.t()[idx.long()]


def with_zero_row(embed, idx):
    """embed (D,K), idx (N) with codes of any value -> (embed with a column of zeros appended (D,K+1), idx with every code outside
    0 .. K-1 sent to K): the formulas of this module on the pair are the header's contract for such codes"""
    K = embed.shape[1]
    idx = idx.detach().cpu().long()
    return torch.cat([embed, torch.zeros_like(embed[:, :1])], 1), torch.where((idx < 0) | (idx >= K), torch.full_like(idx, K), idx)


def quantize(z, embed, idx):
    """-> (quantize (N,D), diff ()) at the dtype of z; differentiable in z as the reference's straight-through form is"""
    e = gather(embed, idx).detach()
    return z + (e - z).detach(), (e - z).pow(2).mean()


def stats(z, idx, K):
    """-> (counts (K) int64, sums (D,K)): index_add_ form"""
    counts = torch.zeros(K, dtype=torch.int64).index_add_(0, idx.long(), torch.ones_like(idx, dtype=torch.int64))
    sums = torch.zeros(K, z.shape[1], dtype=z.dtype).index_add_(0, idx.long(), z).t().contiguous()
    return counts, sums


def stats_onehot(z, idx, K):
    """The reference's form: the one-hot matrix, its column sums and z^T @ onehot"""
    onehot = torch.nn.functional.one_hot(idx.long(), K).to(z.dtype)
    return onehot.sum(0), z.t() @ onehot


def update(cluster_size, embed_avg, counts, sums, decay, eps):
    """-> dict(cluster_size, embed_avg, n, s, embed) in fp64"""
    K = cluster_size.numel()
    alpha = 1 - decay
    cs = decay * cluster_size + alpha * counts.to(cluster_size.dtype)
    avg = decay * embed_avg + alpha * sums
    n = cs.sum()
    s = (cs + eps) / (n + K * eps) * n
    return dict(cluster_size=cs, embed_avg=avg, n=n, s=s, embed=avg / s.unsqueeze(0))


def grad_input(z, embed, idx, grad_quantize, grad_diff):
    """grad_quantize (N,D) or None, grad_diff () or None -> (grad_input, the second term t)"""
    t = torch.zeros_like(z) if grad_diff is None else grad_diff * 2.0 / z.numel() * (z - gather(embed, idx))
    return (t if grad_quantize is None else grad_quantize + t), t


def expected(z, embed, idx, cluster_size, embed_avg, decay, eps):
    """Everything a training forward produces, in fp64 from the fp32 values given -> dict, with the bounds under 'bound'"""
    z, embed, cluster_size, embed_avg = _f64(z), _f64(embed), _f64(cluster_size), _f64(embed_avg)
    idx = idx.detach().cpu().long()
    K = embed.shape[1]
    alpha = 1 - decay
    q, diff = quantize(z, embed, idx)
    counts, sums = stats(z, idx, K)
    up = update(cluster_size, embed_avg, counts, sums, decay, eps)
    _, abs_sums = stats(z.abs(), idx, K)
    b_sums = 1.01 * U * counts.double().unsqueeze(0) * abs_sums
    b_cs = 1.01 * 3 * U * (decay * cluster_size.abs() + alpha * counts.double())
    b_avg = 1.01 * (3 * U * (decay * embed_avg.abs() + alpha * sums.abs()) + alpha * b_sums)
    s = up["s"].unsqueeze(0)
    b_embed = b_avg / s + up["embed_avg"].abs() / s * (R_S + 1.01 * U)
    bound = dict(sums=b_sums, diff=4 * U * diff, cluster_size=b_cs, embed_avg=b_avg, embed=b_embed)
    return dict(quantize=q, diff=diff, counts=counts, sums=sums, bound=bound, **up)


def grad_bound(grad_quantize, term):
    g = torch.zeros_like(term) if grad_quantize is None else grad_quantize.abs()
    return 1.01 * U * (g + 4 * term.abs())


def ratio(got, want, bound):
    """The largest |got - want| / bound over the entries with a bound; where the bound is 0, got must be exactly want (AssertionError)"""
    got, want = _f64(got), _f64(want)
    bound = torch.as_tensor(bound, dtype=torch.float64)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    assert torch.isfinite(got).all()
    closed = bound == 0
    assert (got[closed] == want[closed]).all(), "a result without a bound must be exact"
    if closed.all():
        return 0.0
    return float(((got - want).abs()[~closed] / bound[~closed]).max())


def check(name, got, want, bound, record=None):
    r = ratio(got, want, bound)
    print(f"{name}: largest error / bound {r:.4f}")
    if record is not None:
        key = name.split()[-1]
        record[key] = max(record.get(key, 0.0), r)
    assert r <= 1.0, (name, r)
    return r
