"""worker of tests/test_vq_train_cpu.py::test_sum_over_ranks_across_ranks (gloo, 2 ranks)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from pixelsynth_amd import distributed as D  # noqa: E402

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
assert world == 2
# each rank holds the statistics of its half of the rows; both end with those of all rows
gen = torch.Generator().manual_seed(3)
N, Dm, K = 40, 5, 7
z = torch.randn(N, Dm, generator=gen, dtype=torch.float64)
idx = torch.randint(0, K, (N,), generator=gen)


def stats(rows):
    counts = torch.zeros(K, dtype=torch.int32).index_add_(0, idx[rows], torch.ones(len(rows), dtype=torch.int32))
    sums = torch.zeros(K, Dm, dtype=torch.float64).index_add_(0, idx[rows], z[rows]).t().contiguous()
    return counts, sums


half = torch.arange(N)[rank * N // 2:(rank + 1) * N // 2]
other = torch.arange(N)[(1 - rank) * N // 2:(2 - rank) * N // 2]
counts, sums = stats(half)
got = D.sum_over_ranks(counts, sums)
assert got[0] is counts and got[1] is sums
oc, os_ = stats(other)
mine = stats(half)
assert torch.equal(counts, mine[0] + oc) and counts.dtype == torch.int32 and int(counts.sum()) == N
# (two terms: the order of the ranks cannot show)
assert torch.equal(sums, mine[1] + os_)
assert D.sum_over_ranks() == ()
if rank == 0:
    print("ok")
dist.destroy_process_group()
