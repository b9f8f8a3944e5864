"""The measuring protocol of the *_time.py tools: device events around a call, rounds of alternating routes, device times by kernel
name under torch's profiler.  numpy and torch only, nothing of pixelsynth_amd; tests/test_tools_measure_*.py pin it."""
import numpy as np
import torch


def event_ms(fn):
    """ms of fn() between two device events, on a device synchronised before the first and waited for after the second"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(routes, rounds, calls, warm=3):
    """routes {name: callable}; -> {name: the medians of `rounds` rounds of `calls` event-timed calls, in ms}, the routes taking turns
    call by call, after `warm` calls of each that are not kept"""
    for _ in range(warm):
        for fn in routes.values():
            event_ms(fn)
    medians = {name: [] for name in routes}
    for _ in range(rounds):
        times = {name: [] for name in routes}
        for _ in range(calls):
            for name, fn in routes.items():
                times[name].append(event_ms(fn))
        for name in routes:
            medians[name].append(float(np.median(times[name])))
    return medians


def span(v):
    return [round(min(v), 4), round(max(v), 4)]


def looped_ms(fn, iters, warm):
    """ms per call of `iters` calls between one pair of device events, after `warm` calls and a synchronise"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def device_events(fn, calls):
    """[(name, device ms)] of what `calls` calls of fn run on the device, in the order of torch's profiler; [] where it records none"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return [(ev.name, ev.device_time / 1e3) for ev in prof.events()
            if ev.device_type == torch.autograd.DeviceType.CUDA and ev.device_time > 0]


def kernel_medians(events, names):
    """{name: median ms, rounded to 4} over events [(event name, ms)].  The first entry of `names` found in an event's name owns the
    event, so a name that contains another stands before it (k_stats_finish before k_stats); an event with none of them is dropped"""
    times = {}
    for event, ms in events:
        k = next((k for k in names if k in event), None)
        if k is not None:
            times.setdefault(k, []).append(ms)
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}


def marked(fn, name):
    """fn wrapped in a torch.profiler.record_function range `name`: what by_range sorts device events by"""
    def wrapper(*a, **k):
        with torch.profiler.record_function(name):
            return fn(*a, **k)
    return wrapper


def range_of(ev, prefix):
    """The nearest record_function range whose name begins with `prefix` around the CPU event `ev` (its name without the prefix), or None"""
    while ev is not None:
        if ev.name.startswith(prefix):
            return ev.name[len(prefix):]
        ev = ev.cpu_parent
    return None


def by_range(fn, calls, prefix):
    """[(range, backward, kernel name, device ms)] of what `calls` calls of fn run on the device under torch's profiler.  range: the
    marked range (marked(), names beginning with `prefix`) around the operation that launched the kernel; for a kernel of the backward
    pass -- launched outside every range -- the range of the forward operation it differentiates, found through the profiler's sequence
    numbers (backward True); None where neither gives one."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU]
    forward = {}            # sequence number of a forward operation -> its range
    for e in events:
        r = range_of(e, prefix)
        if r is not None and getattr(e, "sequence_nr", -1) >= 0 and getattr(e, "scope", 0) == 0:
            forward.setdefault(e.sequence_nr, r)
    out = []
    for e in events:
        kernels = getattr(e, "kernels", None) or []
        if not kernels:
            continue
        r, backward, up = range_of(e, prefix), False, e
        while r is None and up is not None:
            if getattr(up, "sequence_nr", -1) >= 0 and up.sequence_nr in forward and "Backward" in up.name:
                r, backward = forward[up.sequence_nr], True
            up = up.cpu_parent
        out.extend((r, backward, k.name, k.duration / 1e3) for k in kernels)
    return out
