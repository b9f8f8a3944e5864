"""Scoring and ranking the best-of-N candidates of a view on the device (the opt-in route of ZbufferModelPts.get_best_sample,
rank_on="device"): csrc/rank.hip behind include/pixelsynth_rank.h.

The host route scores one candidate at a time (reference: models/z_buffermodel.py:254-276): the image goes down to numpy, is read as an
(S,S,3) picture, quantised, resized by Pillow, normalised, goes up again and through the classifier as a batch of one; the
discriminator sees the candidate next to the same input image N times over.  Here the N candidates stay where they are:

    classifier_input   (N,3,S,S) -> the classifier's (N,3,T,T) input: the host's lines bit for bit (Pillow's BILINEAR resample restated)
    entropy            logits (N,C) -> -sum p log p of the fp32 softmax
    hinge_fake         the last patch map of each discriminator scale -> D_Fake per candidate (GANLoss "hinge", fake side)
    select             the rank rule of rank_samples -> the winner's index, on the device
    score_candidates   the four of them around ONE forward of the classifier and ONE of the discriminator, on the N fakes alone

Best-of-N PER VIEW for a batch of B views (get_best_sample's rank_scope="view": csrc/rank_groups.hip behind
include/pixelsynth_rank_groups.h) scores the N * B candidates with score_candidates, in chunks, and then

    select_groups      the rank rule in every view's own N candidates -> B winner indices, on the device
    take_groups        the B winners out of the N * B candidates, the indices read where they are

The numpy restatements the tests pin them to (pil_bilinear_tables, classifier_input_reference, select_reference,
select_groups_reference) live here too.
"""
import functools
import math

import numpy as np
import torch

from . import _lib

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)     # the classifier's normalisation (z_buffermodel.py:258)
MAX_SIDE, MAX_N = 1024, 1024                                 # PS_RANK_MAX_SIDE, PS_RANK_MAX_N
MAX_GROUPS = 65535                                           # PS_RANK_MAX_GROUPS
LAYOUTS = ("candidate_major", "group_major")
SCORE_CHUNK = 64                                             # candidates per forward of the scorers where a cap is asked for (score_candidates)
PRECISION_BITS = 32 - 8 - 2


@functools.lru_cache(maxsize=None)
def pil_bilinear_tables(S, T):
    """Pillow's BILINEAR resample of S samples to T (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc) ->
    (bounds (T,2) int32: first input index and number of taps per output index, coeffs (T,ksize) int32: the taps' weights in 22-bit
    fixed point, zero past the last tap).  The triangle filter has support max(S/T, 1); everything is worked out in double, in
    Pillow's order of operations."""
    if not (1 <= S <= MAX_SIDE and 1 <= T <= MAX_SIDE):
        raise ValueError(f"pil_bilinear_tables: S = {S}, T = {T}, expected 1 .. {MAX_SIDE}")
    scale = S / T
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = np.zeros((T, 2), np.int32), np.zeros((T, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(T):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), S) - xmin
        ww = 0.0
        for x in range(count):
            w = max(1.0 - abs((x + xmin - center + 0.5) * ss), 0.0)
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            kk[xx, :count] /= ww
        bounds[xx] = xmin, count
    coeffs = np.where(kk < 0, -0.5 + kk * (1 << PRECISION_BITS), 0.5 + kk * (1 << PRECISION_BITS)).astype(np.int32)   # (int): truncation
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


@functools.lru_cache(maxsize=None)
def norm_table():
    """(3,256) fp32: [c][u] = ((u / 255 - mean_c) / std_c) formed as the host route forms it (_entropy_score: fp32 arrays throughout)"""
    u = np.arange(256).astype(np.float32)[:, None] / 255.0
    t = np.ascontiguousarray(((u - np.array(MEAN, np.float32)) / np.array(STD, np.float32)).T)
    assert t.dtype == np.float32
    t.setflags(write=False)
    return t


def quantise_reference(x):
    """fp32 array -> uint8 as ps_rank_classifier_input defines it: trunc(((x * .5) + .5) * 255) in fp32, for x in [-1,1] what numpy's
    .astype(uint8) gives; outside, the value clamped to [-2^31, 2^31 - 128], truncated, its low byte; NaN -> 0."""
    v = (np.asarray(x, np.float32) * np.float32(.5) + np.float32(.5)) * np.float32(255)
    v = np.where(np.isnan(v), np.float32(-2147483648.0), np.clip(v, np.float32(-2147483648.0), np.float32(2147483520.0)))
    return (v.astype(np.int64) & 255).astype(np.uint8)


def _resample_axis1(img, bounds, coeffs):
    """One pass of the resample along axis 1 of a uint8 (rows, S, 3) image -> (rows, T, 3) uint8"""
    out = np.empty((img.shape[0], bounds.shape[0], img.shape[2]), np.uint8)
    wide = img.astype(np.int64)
    for i, (lo, count) in enumerate(bounds):
        ss = (1 << (PRECISION_BITS - 1)) + np.tensordot(wide[:, lo:lo + count], coeffs[i, :count].astype(np.int64), axes=([1], [0]))
        out[:, i] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resize_reference(raw, T):
    """uint8 (S,S,3) -> (T,T,3): Image.fromarray(raw).resize((T,T), Image.BILINEAR) restated -- the horizontal pass into uint8, then
    the vertical one"""
    bounds, coeffs = pil_bilinear_tables(raw.shape[0], T)
    horizontal = _resample_axis1(raw, bounds, coeffs)
    return _resample_axis1(horizontal.transpose(1, 0, 2), bounds, coeffs).transpose(1, 0, 2)


def classifier_input_reference(imgs, T=224):
    """numpy (N,3,S,S) fp32 -> (the classifier's input (N,3,T,T) fp32, the resized bytes (N,T,T,3) uint8): what _entropy_score does
    to one candidate on the host, restated without Pillow."""
    imgs = np.asarray(imgs, np.float32)
    N, C, S, S2 = imgs.shape
    if C != 3 or S != S2:
        raise ValueError(f"classifier_input_reference: expected (N,3,S,S), got {imgs.shape}")
    table = norm_table()
    out, resized = np.empty((N, 3, T, T), np.float32), np.empty((N, T, T, 3), np.uint8)
    for n in range(N):
        resized[n] = resize_reference(quantise_reference(imgs[n].reshape(S, S, 3)), T)   # (the reference's reshape, not a permute)
        for c in range(3):
            out[n, c] = table[c][resized[n, :, :, c]]
    return out, resized


def ranks_reference(values):
    """rank of every element = how many sort before it: ascending, the lower index first among equals, NaN after every number"""
    v = np.asarray(values, np.float64)
    order = np.lexsort((np.arange(len(v)), np.where(np.isnan(v), 0.0, v), np.isnan(v)))
    ranks = np.empty(len(v), np.int64)
    ranks[order] = np.arange(len(v))
    return ranks


def select_reference(disc, entr):
    """-> (the index ps_rank_select keeps, disc_rank, entr_rank): rank_samples' rule with the order of equal scores pinned down"""
    n = len(disc)
    disc_rank, entr_rank = ranks_reference(disc), ranks_reference(entr)
    return int(np.argmax((n - 1 - entr_rank) + disc_rank)), disc_rank, entr_rank


def group_strides(groups, n, layout):
    """layout -> (group_stride, cand_stride) of ps_rank_select_groups / ps_rank_take_groups: candidate i of group g lies at
    g * group_stride + i * cand_stride"""
    if layout not in LAYOUTS:
        raise ValueError(f"layout is {layout!r}, expected one of {LAYOUTS}")
    return (1, groups) if layout == "candidate_major" else (n, 1)


def select_groups_reference(disc, entr, groups, n, layout="candidate_major"):
    """-> (best (groups,), disc_rank, entr_rank (groups * n,) laid out as the scores are): select_reference on every group's own scores"""
    disc, entr = np.asarray(disc).reshape(-1), np.asarray(entr).reshape(-1)
    if len(disc) != groups * n or len(entr) != groups * n or groups < 1 or n < 1:
        raise ValueError(f"select_groups_reference: expected two lists of {groups} * {n} scores, got {len(disc)} and {len(entr)}")
    gs, cs = group_strides(groups, n, layout)
    best, disc_rank, entr_rank = np.empty(groups, np.int64), np.empty(groups * n, np.int64), np.empty(groups * n, np.int64)
    for g in range(groups):
        at = g * gs + np.arange(n) * cs
        best[g], disc_rank[at], entr_rank[at] = select_reference(disc[at], entr[at])
    return best, disc_rank, entr_rank


# ---------------------------------------------------------------- the device wrappers
_TABLES = {}    # (S, T, device index) -> (bounds, coeffs, norm) on that device: uploaded once


def _device_tables(S, T, device):
    key = (S, T, device.index)
    t = _TABLES.get(key)
    if t is None:
        bounds, coeffs = pil_bilinear_tables(S, T)
        t = _TABLES[key] = tuple(torch.from_numpy(a.copy()).to(device) for a in (bounds, coeffs, norm_table()))
    return t


def _fp32(name, t, dim):
    _lib.require_cuda(t)
    if t.dtype != torch.float32 or t.dim() != dim:
        raise ValueError(f"{name}: expected a {dim}-d fp32 tensor, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def classifier_input(imgs, T=224, want_bytes=False):
    """(N,3,S,S) fp32 on the device -> the classifier's input (N,3,T,T) fp32 [, the resized bytes (N,T,T,3) uint8]; one launch"""
    imgs = _fp32("classifier_input", imgs, 4)
    N, C, S, S2 = imgs.shape
    if C != 3 or S != S2 or not (1 <= S <= MAX_SIDE and 1 <= T <= MAX_SIDE) or N < 1:
        raise ValueError(f"classifier_input: expected (N,3,S,S) with N >= 1 and S, T in 1 .. {MAX_SIDE}, got {tuple(imgs.shape)}, T = {T}")
    with torch.cuda.device(imgs.device):
        bounds, coeffs, norm = _device_tables(S, T, imgs.device)
        out = torch.empty(N, 3, T, T, dtype=torch.float32, device=imgs.device)
        resized = torch.empty(N, T, T, 3, dtype=torch.uint8, device=imgs.device) if want_bytes else None
        _lib.call("ps_rank_classifier_input", imgs, N, S, T, bounds, coeffs, coeffs.shape[1], norm, out, resized)
    return (out, resized) if want_bytes else out


def entropy(logits):
    """(N,C) fp32 on the device -> (N,) fp32: the entropy of every row's softmax; one launch"""
    logits = _fp32("entropy", logits, 2)
    N, C = logits.shape
    if N < 1 or C < 1:
        raise ValueError(f"entropy: expected a non-empty (N,C), got {tuple(logits.shape)}")
    with torch.cuda.device(logits.device):
        out = torch.empty(N, dtype=torch.float32, device=logits.device)
        _lib.call("ps_rank_entropy", logits, N, C, out)
    return out


def hinge_fake(map0, map1):
    """The last patch maps of the two discriminator scales, (N,1,h0,w0) and (N,1,h1,w1) fp32 -> D_Fake (N,) fp32; one launch"""
    map0, map1 = _fp32("hinge_fake", map0, 4), _fp32("hinge_fake", map1, 4)
    N = map0.shape[0]
    if map1.shape[0] != N or map0.shape[1] != 1 or map1.shape[1] != 1 or N < 1 or map0.numel() == 0 or map1.numel() == 0:
        raise ValueError(f"hinge_fake: expected (N,1,h0,w0) and (N,1,h1,w1), got {tuple(map0.shape)} and {tuple(map1.shape)}")
    with torch.cuda.device(map0.device):
        out = torch.empty(N, dtype=torch.float32, device=map0.device)
        _lib.call("ps_rank_hinge_fake", map0, map0.numel() // N, map1, map1.numel() // N, N, out)
    return out


def select(disc, entr, want_ranks=False):
    """disc (n), entr (n) fp32 on the device -> the kept index as a (1,) int64 device tensor [, disc_rank, entr_rank (n) int32]"""
    disc, entr = _fp32("select", disc, 1), _fp32("select", entr, 1)
    n = disc.shape[0]
    if entr.shape[0] != n or not 1 <= n <= MAX_N:
        raise ValueError(f"select: expected two lists of 1 .. {MAX_N} scores, got {n} and {entr.shape[0]}")
    with torch.cuda.device(disc.device):
        best = torch.empty(1, dtype=torch.int32, device=disc.device)
        ranks = [torch.empty(n, dtype=torch.int32, device=disc.device) for _ in range(2)] if want_ranks else [None, None]
        _lib.call("ps_rank_select", disc, entr, n, best, *ranks)
    return (best.long(), *ranks) if want_ranks else best.long()


def select_groups(disc, entr, groups, n, layout="candidate_major", want_ranks=False):
    """disc, entr (groups * n) fp32 on the device, candidate i of group g where `layout` puts it (group_strides) -> the kept index of
    every group as a (groups,) int32 device tensor [, disc_rank, entr_rank (groups * n) int32, laid out as the scores]; one launch"""
    disc, entr = _fp32("select_groups", disc, 1), _fp32("select_groups", entr, 1)
    gs, cs = group_strides(groups, n, layout)
    if not (1 <= n <= MAX_N and 1 <= groups <= MAX_GROUPS) or disc.shape[0] != groups * n or entr.shape[0] != groups * n:
        raise ValueError(f"select_groups: expected two lists of groups * n scores with n in 1 .. {MAX_N} and groups in 1 .. {MAX_GROUPS}, "
                         f"got groups = {groups}, n = {n} and lists of {disc.shape[0]} and {entr.shape[0]}")
    with torch.cuda.device(disc.device):
        best = torch.empty(groups, dtype=torch.int32, device=disc.device)
        ranks = [torch.empty(groups * n, dtype=torch.int32, device=disc.device) for _ in range(2)] if want_ranks else [None, None]
        _lib.call("ps_rank_select_groups", disc, entr, groups, n, gs, cs, best, *ranks)
    return (best, *ranks) if want_ranks else best


def take_groups(src, best, n, layout="candidate_major"):
    """src (groups * n, ...) fp32 on the device, best (groups,) int32 on the device (select_groups': an index outside 0 .. n-1 is
    clamped into it) -> (groups, *src.shape[1:]): item best[g] of every group; one launch, the indices are read where they are"""
    _lib.require_cuda(src, best)
    if src.dtype != torch.float32 or src.dim() < 1 or best.dtype != torch.int32 or best.dim() != 1:
        raise ValueError(f"take_groups: expected fp32 items and a 1-d int32 index, got {tuple(src.shape)} {src.dtype} and "
                         f"{tuple(best.shape)} {best.dtype}")
    src, best, groups = src.contiguous(), best.contiguous(), best.shape[0]
    gs, cs = group_strides(groups, n, layout)
    item = src[0].numel() if src.shape[0] else 0
    if not (1 <= n <= MAX_N and 1 <= groups <= MAX_GROUPS) or src.shape[0] != groups * n or item < 1:
        raise ValueError(f"take_groups: expected groups * n non-empty items with n in 1 .. {MAX_N} and groups in 1 .. {MAX_GROUPS}, got "
                         f"{groups} indices, n = {n} and items {tuple(src.shape)}")
    with torch.cuda.device(src.device):
        out = torch.empty((groups,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
        _lib.call("ps_rank_take_groups", src, best, groups, n, gs, cs, item, out)
    return out


# ---------------------------------------------------------------- the two scorers on a batch of candidates
def _discriminator(netD):
    """The multiscale discriminator module inside pixelsynth_amd.losses.DiscriminatorLoss (or the reference's class), its loss object"""
    base = getattr(netD, "netD", None)
    return getattr(base, "netD", None), getattr(base, "criterionGAN", None)


def can_score_on_device(netD, classifier, imgs=None):
    """Whether score_candidates stands for the host route's two scorers: the discriminator is reachable as netD.netD.netD, its loss is
    GANLoss in hinge mode, the classifier is a module -- and, given the candidates, they are (N,3,S,S) fp32 on the GPU."""
    disc, crit = _discriminator(netD)
    ok = isinstance(disc, torch.nn.Module) and isinstance(classifier, torch.nn.Module) and getattr(crit, "gan_mode", None) == "hinge"
    if ok and imgs is not None:
        ok = (torch.is_tensor(imgs) and imgs.is_cuda and imgs.dtype == torch.float32 and imgs.dim() == 4 and imgs.shape[1] == 3
              and imgs.shape[2] == imgs.shape[3] and 1 <= imgs.shape[2] <= MAX_SIDE)
    return bool(ok)


@torch.no_grad()
def score_candidates(imgs, netD, classifier, chunk=None):
    """imgs (N,3,S,S) fp32 on the device -> (disc (N,), entr (N,)) fp32 device tensors, the scores get_best_sample ranks with; nothing
    comes down to the host.  One classifier_input launch, one forward of the classifier on the N inputs, one entropy launch; one
    forward of the multiscale discriminator on the N candidates alone (every layer of it works per sample, and the input image's half
    of the host route's batch is read by nobody), one hinge_fake launch.
    chunk: None -- the single pass above (the B = 1 route).  A number: the passes run on at most `chunk` candidates at a time and the
    score vectors are concatenated (a candidate's scores do not depend on its neighbours: every layer works per sample).  It is a cap
    on memory, not a tuning knob: the N * B candidates of per-view ranking, 50 x 16 say, would put several GB into the discriminator's
    first layers at once (64 channels of 128 x 128 fp32 per candidate and layer: 4 MB each, 0.27 GB at 64 candidates, 3.4 GB at 800).
    The per-view route passes opt.rank_chunk, SCORE_CHUNK = 64 where it is unset -- a figure chosen from these activation sizes, not
    measured."""
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"score_candidates: chunk = {chunk}, expected >= 1 (or None: one pass)")
    if not can_score_on_device(netD, classifier, imgs):
        raise RuntimeError("score_candidates: needs netD.netD.netD with a hinge GANLoss, a classifier module and (N,3,S,S) fp32 "
                           "candidates on the GPU (can_score_on_device); there is no fallback here")
    if chunk is None or imgs.shape[0] <= int(chunk):
        return _score_pass(imgs, netD, classifier)
    parts = [_score_pass(imgs[s:s + int(chunk)], netD, classifier) for s in range(0, imgs.shape[0], int(chunk))]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _score_pass(imgs, netD, classifier):
    """score_candidates' single pass on candidates it has checked"""
    entr = entropy(classifier(classifier_input(imgs)).float())
    disc, _ = _discriminator(netD)
    maps = [p[-1] if isinstance(p, (list, tuple)) else p for p in disc(imgs)]   # the last entry of every scale counts (GANLoss)
    if len(maps) != 2:
        raise RuntimeError(f"score_candidates: the discriminator has {len(maps)} scales, ps_rank_hinge_fake takes two")
    return hinge_fake(maps[0], maps[1]), entr
