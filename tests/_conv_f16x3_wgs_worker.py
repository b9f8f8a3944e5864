"""Worker of tests/test_conv_f16x3_walk_gpu.py: PS_CONV_WGS is read once per process, so another grid needs a fresh one.  Runs the
small set of tests/_conv_f16x3_ref.wgs_cases() under the PS_CONV_WGS of its environment and writes every output (and overflow flag) to
the .npz named on the command line.  Judges nothing: the parent holds the outputs against fp64 and against its own grid's."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _conv_f16x3_ref as M  # noqa: E402  (beside this file)


def main(out):
    dev = torch.device("cuda", 0)
    res = {"wgs": np.int64(M.wgs_in_force())}
    for c in M.wgs_cases():
        y, flag = M.wgs_case_run(M.wgs_case_inputs(c, dev))
        res[M.wgs_case_name(c)] = y.contiguous().cpu().numpy()
        res[M.wgs_case_name(c) + "_flag"] = flag.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
