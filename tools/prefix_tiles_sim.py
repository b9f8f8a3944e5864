"""CPU model of the work of the prefix pass's products (k_gemm_ws, csrc/lmconv_grid.hip) on the bench's own plans: what the
stages' own item lists (prefix_compact) and the exact dependency sets (prefix_exact) take away, and the SQ_INSTS_MFMA per launch a
`rocprofv3 --pmc SQ_INSTS_MFMA` pass should show for each setting.  Reads oracle/ only (the C oracle's projection, splat and
generation orders; oracle/prefix_cone_oracle.py for the start ranks and the exact sets); needs no GPU.

    python tools/prefix_tiles_sim.py [--views 128] [--every 1] [--jobs 8]

The item lists are laid out as k_perm_sort / _scan / _scatter lay them: frame ranges of 64 (ZbufferModelPts.PREFIX_STREAMS = 2), per range
one share of the frames per XCD, inside a share the tap sets heaviest first (number of open taps, then the 9-bit set), frame, rank;
ranks behind a frame's own end in the last bin; npre = the batch's largest first sampled position.  A tile is 64 positions (one
workgroup), a wave 16; a workgroup runs when one of its items is evaluated and then costs its set-up and post op ("2") plus one
(tap, chain) sequence per tap that is open for one of its evaluated items (notebook, round 6); a wave issues MFMAs for a tap that is open
for one of ITS evaluated items: 400 / 200 / 100 per (wave, tap) for conv_out / conv_input / dilated (k_gemm_ws<0 / 1 / 2>).
--every n: every n-th view only (shares of 8 / n frames), for a quick look."""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import c_oracle, prefix_cone_oracle as pc   # noqa: E402

KINDS = ("conv_input", "conv_out", "dilated")
MFMA_PER_UNIT = {"conv_input": 200, "conv_out": 400, "dilated": 100}
WS_KERNEL = {"conv_input": "k_gemm_ws<1>", "conv_out": "k_gemm_ws<0>", "dilated": "k_gemm_ws<2>"}
G_SKIP = pc.G_SKIP


def stage_kind(s):
    return "conv_input" if s < 15 else "conv_out" if s < 29 else "dilated"


def plan_of_view(args):
    """One view of bench.make_inputs -> order, tap sets by rank (dilation 1 / 2), the frame's end, start ranks, exact sets."""
    depth, img, K, Kinv, Pinv, RT2, exact = args
    S = 256
    sampler = c_oracle.project_pts(depth, K, Kinv, Pinv, RT2, S)
    bg = c_oracle.splat_forward(np.ascontiguousarray(sampler.transpose(0, 2, 1)), img.reshape(1, 3, -1), S, K=128)["bg"][0]
    info = c_oracle.masks_for_background(bg, 32)
    order = (info["order"][:, 0] * 32 + info["order"][:, 1]).astype(np.int64)
    sampled = info["bg32"].reshape(-1)[order] != 0
    end = int(sampled.argmax()) if sampled.any() else 1024
    und, dil = info["mask_undilated"][0], info["mask_dilated"][0]
    pats = []
    for mask, d in ((und, 1), (dil, 2)):
        y, x = order // 32, order % 32
        p = np.zeros(1024, np.int64)
        for t in range(9):
            yy, xx = y + d * (t // 3 - 1), x + d * (t % 3 - 1)
            p |= ((mask[t, order] != 0) & (yy >= 0) & (yy < 32) & (xx >= 0) & (xx < 32)).astype(np.int64) << t
        pats.append(p)
    starts = pc.prefix_starts(order, und, dil, 32, 32, end)
    sets = np.stack(pc.exact_need_sets(order, und, dil, 32, 32, end)) if exact and end > 0 else None
    return dict(end=end, pats=pats, starts=starts, sets=sets)


def bins():
    """place of a tap set in the sort: number of open taps descending, then the set (make_perm_bins)."""
    b, n = np.zeros(512, np.int64), 0
    for pcnt in range(9, -1, -1):
        for p in range(512):
            if bin(p).count("1") == pcnt:
                b[p] = n
                n += 1
    return b


def measure(pat, live, skip_tap):
    """pat / live by position of one launch's list (a multiple of 64 positions, padded dead) -> tiles, sum(2 + taps), (wave, tap) units."""
    taps = ((pat[:, None] >> np.arange(9)) & 1).astype(bool) & live[:, None]
    w = taps.reshape(-1, 16, 9).any(1)                       # (waves, 9)
    wl = live.reshape(-1, 16).any(1)
    units = int(w.sum()) + (int(wl.sum()) if skip_tap else 0)
    t = w.reshape(-1, 4, 9).any(1)
    tl = wl.reshape(-1, 4).any(1)
    return int(tl.sum()), int((2 + t.sum(1) + (1 if skip_tap else 0))[tl].sum()), units


def pad64(a, fill):
    n = -len(a) % 64
    return np.concatenate([a, np.full(n, fill, a.dtype)]) if n else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--no-exact", action="store_true", help="skip the exact sets (minutes of numpy per 128 views)")
    o = ap.parse_args()
    import bench
    _, host = bench.make_inputs(0, o.views, "cpu")
    cam = host["cam"]
    ids = list(range(0, o.views, o.every))
    jobs = [(host["depth"][v:v + 1], host["img"][v:v + 1], cam["K"][v:v + 1], cam["Kinv"][v:v + 1], cam["Pinv"][v:v + 1], host["RT2"][v:v + 1],
             not o.no_exact) for v in ids]
    with Pool(o.jobs) as pool:
        plans = pool.map(plan_of_view, jobs)
    V = len(plans)
    npre = max(p["end"] for p in plans)
    nranges = 2 if V >= 64 and V % 16 == 0 else 1      # (ZbufferModelPts._prefix_split)
    per_range = V // nranges
    parts = 8 if per_range >= 16 and per_range % 8 == 0 else 1
    fpp = per_range // parts
    place = bins()
    print(f"{V} views, npre = {npre}, {nranges} frame range(s) of {per_range}, {parts} share(s) of {fpp} frames")
    layouts = ["current", "compacted"] + ([] if o.no_exact else ["exact", "exact + compacted"])
    tot = {(k, l): np.zeros(4, np.int64) for k in KINDS for l in layouts}      # tiles, sum(2 + taps), units, items
    launches = {k: 0 for k in KINDS}
    for rg in range(nranges):
        frames = plans[rg * per_range:(rg + 1) * per_range]
        lists = []                                               # per mask kind: per share (frame, rank, pat) in list order
        for kind in range(2):
            shares = []
            for sh in range(parts):
                fr, rk, pt, key = [], [], [], []
                for fl in range(sh * fpp, (sh + 1) * fpp):
                    p = frames[fl]
                    r = np.arange(npre)
                    dead = r >= p["end"]
                    fr.append(np.full(npre, fl)); rk.append(r); pt.append(p["pats"][kind][:npre])
                    key.append(np.where(dead, 511, place[p["pats"][kind][:npre]]))
                fr, rk, pt, key = (np.concatenate(a) for a in (fr, rk, pt, key))
                idx = np.lexsort((rk, fr, key))
                shares.append((fr[idx], rk[idx], pt[idx]))
            lists.append(shares)
        ends = np.array([p["end"] for p in frames])
        sets = np.zeros((per_range, pc.N_EVAL, npre), bool)        # exact sets by (frame, stage, rank), nothing behind a frame's end
        if not o.no_exact:
            for fl, p in enumerate(frames):
                if p["sets"] is not None:
                    sets[fl, :, :p["end"]] = p["sets"]
        for s in range(1, pc.N_EVAL):
            k = stage_kind(s)
            launches[k] += 1
            skip = k == "conv_input" and G_SKIP[s - 1] >= 0
            starts = np.array([p["starts"][s] for p in frames])
            for exact in ([False] if o.no_exact else [False, True]):
                cur_pat, cur_live, cmp_pat, cmp_live = [], [], [], []
                for fr, rk, pt in lists[1 if k == "dilated" else 0]:
                    live = sets[fr, s, rk] if exact else (rk >= starts[fr]) & (rk < ends[fr])
                    cur_pat.append(pt); cur_live.append(live)
                    kept = pt[live]                              # the stage's own list of this share, at the share's own base:
                    cmp_pat.append(pad64(kept, 0) if parts > 1 else kept)              # its last tile is padded
                    cmp_live.append(pad64(np.ones(len(kept), bool), False) if parts > 1 else np.ones(len(kept), bool))
                cp, cl = pad64(np.concatenate(cur_pat), 0), pad64(np.concatenate(cur_live), False)
                tot[(k, "exact" if exact else "current")] += np.array(measure(cp, cl, skip) + (int(cl.sum()),))
                cp, cl = pad64(np.concatenate(cmp_pat), 0), pad64(np.concatenate(cmp_live), False)
                tot[(k, "exact + compacted" if exact else "compacted")] += np.array(measure(cp, cl, skip) + (int(cl.sum()),))
    print(f"{'stage kind':11s} {'layout':18s} {'items/step':>11s} {'tiles':>8s} {'sum(2+taps)':>12s} {'(wave,tap)':>11s} {'MFMA/launch':>12s}   relative to current")
    for k in KINDS:
        base = tot[(k, "current")].astype(float)
        for l in layouts:
            t = tot[(k, l)]
            per_launch = t[2] / launches[k]
            rel = " ".join(f"{x:.3f}" for x in (t[3] / base[3], t[0] / base[0], t[1] / base[1], t[2] / base[2]))
            print(f"{k:11s} {l:18s} {t[3]:11d} {t[0]:8d} {t[1]:12d} {t[2]:11d} {per_launch * MFMA_PER_UNIT[k]:12.0f}   {rel}   ({WS_KERNEL[k]}: {per_launch:.0f} units x {MFMA_PER_UNIT[k]})")


if __name__ == "__main__":
    main()
