"""Measurement: build_ar_plan per route -- order_on="host" (mask down, ps_ar_plan on host threads, orders up) against order_on="device"
(ps_plan_order on the masks where they are, orders down) -- on the background masks of a real synthetic splat.

    python tools/plan_route_time.py [V ...]        (default: 16 128)

The masks of V views are made once, outside the timed part.  Per route: WARM calls, then CALLS timed calls, each from a synchronised
device to the returned plan (build_ar_plan synchronises before it returns); the routes alternate call by call, in one process.  Wall time
per call as min / median / max, and for the device route the kernel alone between two events.  One JSON line per V at the end."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from pixelsynth_amd import _lib  # noqa: E402
from pixelsynth_amd.ar_plan import build_ar_plan  # noqa: E402

WARM, CALLS = 3, 10


def kernel_ms(bgm, G=32):
    """ps_plan_order alone, event-timed, CALLS launches one by one -> their times"""
    B, S, _ = bgm.shape
    as_u8 = bgm.view(torch.uint8) if bgm.dtype == torch.bool else bgm
    order = torch.empty(B, G * G, dtype=torch.int32, device=bgm.device)
    region = torch.empty(B, G * G, dtype=torch.uint8, device=bgm.device)
    first, counts = (torch.empty(B, dtype=torch.int32, device=bgm.device) for _ in range(2))
    out = []
    for rep in range(WARM + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call("ps_plan_order", as_u8, B, S, G, order, region, first, counts)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out[WARM:]


def main(argv):
    views = [int(a) for a in argv] or [16, 128]
    device = torch.device("cuda", 0)
    model = bench.build_model(device)
    for V in views:
        d, _ = bench.make_inputs(0, V, device)
        _, bgm = model.pts_transformer.forward_justpts(d["img"], d["depth"], d["K"], d["Kinv"], d["P"], d["Pinv"], d["RT2"], d["RT2inv"])
        bgm = bgm.contiguous()
        torch.cuda.synchronize()
        wall = {"host": [], "device": []}
        for rep in range(WARM + CALLS):
            for route in wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                plan = build_ar_plan(bgm, 32, order_on=route)
                t1 = time.perf_counter()
                if rep >= WARM:
                    wall[route].append(1e3 * (t1 - t0))
                del plan
        kern = kernel_ms(bgm)
        stat = lambda x: [round(float(f(x)), 3) for f in (np.min, np.median, np.max)]
        rec = dict(V=V, calls=CALLS, host_wall_ms=stat(wall["host"]), device_wall_ms=stat(wall["device"]), device_kernel_ms=stat(kern),
                   background_fraction=round(float(bgm.float().mean()), 3), cpus=len(os.sched_getaffinity(0)))
        print("V=%d  build_ar_plan wall per call (min / median / max of %d): host %.2f / %.2f / %.2f ms, device %.2f / %.2f / %.2f ms; "
              "ps_plan_order alone %.3f / %.3f / %.3f ms" % (V, CALLS, *rec["host_wall_ms"], *rec["device_wall_ms"], *rec["device_kernel_ms"]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
