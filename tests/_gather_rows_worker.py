"""worker of tests/test_metrics_cpu.py::test_gather_rows_across_ranks (gloo, 2 ranks)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

from pixelsynth_amd import distributed as D  # noqa: E402

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
for n, k in ((7, 6), (2, 3), (1, 6), (0, 2)):
    rows = np.random.RandomState(11 + n).randn(k, n)
    mine = D.shard_views(n, rank, world)
    got = D.gather_rows(rows[:, mine], n)
    assert got.shape == (k, n) and got.dtype == np.float64, (got.shape, got.dtype)
    assert np.array_equal(got, rows), (got, rows)
if rank == 0:
    print("ok")
dist.destroy_process_group()
