"""The AR plan of a batch: what the sampler needs on the device -- generation orders, sampled regions, the three kernel masks and
the wavefront schedules -- built from background masks (build_ar_plan, the product path) or from values in the reference's form
(plan_from_reference_args: get_best_sample and sample() as the reference calls them)."""
import collections
import os
import threading

import numpy as np
import torch

from . import _lib
from .lmconv.locally_masked_convolution import compact_mask
from .lmconv.model import TP_MIN_FRAMES, wavefronts

PER_FRAME_PREFIX = os.environ.get("PS_PER_FRAME_PREFIX", "1") != "0"   # plans also carry the schedule of per-frame prefixes (waves_frames)

_PINNED = collections.OrderedDict()
_PINNED_MAX = 12                       # staging buffers kept (four per batch shape): the oldest shapes are released
_PLAN_LOCK = threading.RLock()         # the staging buffers are shared state: one plan is staged at a time per process


def _pinned(name, shape, dtype):
    """Page-locked staging buffers (pageable copies ran at ~0.6 GB/s on the MI355X hosts), kept per (name, shape) in a small
    LRU: callers that vary their batch size do not pile up pinned host memory.  Used under _PLAN_LOCK."""
    key = (name, tuple(shape), dtype)
    t = _PINNED.pop(key, None)
    if t is None:
        t = torch.empty(shape, dtype=dtype, pin_memory=True)
    _PINNED[key] = t
    while len(_PINNED) > _PINNED_MAX:
        _PINNED.popitem(last=False)
    return t


class ARPlan:
    """Device-resident, compact result of get_masks_for_batch for B images (see ps_ar_plan).  order_host / region_host: the
    (B,L) orders (location by rank) and sampled regions (by location) on the host, shape: the (H, W) code grid."""

    def __init__(self, order_loc, region, mask_init, mask_undilated, mask_dilated, order_host, region_host, shape):
        self.order_loc, self.region = order_loc, region
        self.mask_init, self.mask_undilated, self.mask_dilated = mask_init, mask_undilated, mask_dilated
        self.order_host = order_host
        self.H, self.W = shape
        L = self.H * self.W
        # per-frame prefixes: a frame's first SAMPLED position (L: none) -- the observed positions in front of it need no column;
        # the batch's columns start at the first of them (what ps_ar_plan reports as first_step)
        sampled = np.take_along_axis(region_host, order_host.astype(np.int64), 1) != 0
        self.first_steps = np.where(sampled.any(1), sampled.argmax(1), L).astype(np.int32)
        self.first_step = int(self.first_steps.min())
        self.n_sampled = region_host.sum(1).astype(int)
        # the schedule of per-frame prefixes (cols on the device, wave_start on the host) and first_steps on the device: where
        # build_ar_plan made them, None otherwise
        self.waves_frames = self.first_steps_dev = None
        self.background_counts = None    # build_ar_plan(count_background=True): set pixels of every mask (it has them on the host)
        self._waves = None

    @property
    def gen_order(self):
        """list of (L,2) int arrays (row, col) by rank: the reference's gen_order (built on demand)."""
        return [np.stack([o // self.W, o % self.W], 1).astype(np.int64) for o in self.order_host]

    # The wavefront schedule of ONE first step for the whole batch: (cols on the device, wave_start on the host).  A plan that carries
    # the schedule of per-frame prefixes (waves_frames: what the batched paths run) builds this one on first use -- 3.6 of the 9.8 ms of
    # host work per 128-view plan, and only the measurement / parity callers ask for it.
    @property
    def waves(self):
        if self._waves is None:
            self._waves = wavefronts(self.order_host, self.H, self.W, self.first_step, self.order_loc.device)
        return self._waves

    def schedule(self, per_frame):
        """The schedule of an AR run of this plan -> (waves, the prefix keywords of PixelCNNEngine.ar_prefix that go with it).
        per_frame: the caller runs per-frame prefixes where the plan carries their schedule."""
        if per_frame and self.waves_frames is not None:
            return self.waves_frames, dict(first_steps=self.first_steps_dev, max_first_step=int(self.first_steps.max()))
        return self.waves, {}

    def device_tensors(self):
        """The plan's device tensors (the whole-batch schedule only once it has been built)."""
        cols = [w[0] for w in (self._waves, self.waves_frames) if w is not None]
        return [t for t in [self.order_loc, self.region, self.mask_init, self.mask_undilated, self.mask_dilated, self.first_steps_dev] + cols
                if t is not None]


PLAN_ORDER_ROUTES = ("host", "device")


def _order_route(order_on):
    """order_on of build_ar_plan -> "host" / "device"; None: the environment variable PS_PLAN_ORDER (read per call), host by default"""
    route = os.environ.get("PS_PLAN_ORDER", "host") if order_on is None else order_on
    if route not in PLAN_ORDER_ROUTES:
        raise ValueError(f"build_ar_plan: order_on / PS_PLAN_ORDER is {route!r}, expected one of {PLAN_ORDER_ROUTES}")
    return route


def _finish_plan(plan, G, device, first_steps_dev=None):
    """The schedules of a plan whose orders are on the host (both routes of build_ar_plan).  first_steps_dev: the device copy of
    plan.first_steps where the caller has one already; uploaded otherwise."""
    B = len(plan.order_host)
    if PER_FRAME_PREFIX and int(plan.first_steps.max()) > plan.first_step:
        if first_steps_dev is None:
            fs_t = _pinned("first_steps", (B,), torch.int32)
            fs_t.numpy()[:] = plan.first_steps
            first_steps_dev = fs_t.to(device, non_blocking=True)
        plan.first_steps_dev = first_steps_dev
        plan.waves_frames = wavefronts(plan.order_host, G, G, plan.first_step, device, first_steps=plan.first_steps)
    if plan.waves_frames is None or B < TP_MIN_FRAMES:
        plan.waves   # (no per-frame schedule, or a small batch, whose outpaint_planned runs this one: built here, off the AR stream)
    _lib.read_status("ps_order_masks_f32", device)   # synchronises: the staging buffers are free again, and a bad order is an error


def build_ar_plan(background_mask, G=32, device=None, count_background=False, order_on=None):
    """background_mask (B,S,S) bool/uint8 tensor (device or host) -> ARPlan on `device`.
    order_on "host": one device->host copy of the mask (the reference does four, z_buffermodel.py:662-669), the integer work (pooling,
    distance transforms, generation order) in C++ on the host (csrc/host_order.cpp), the orders back up, and the three
    kernel masks built from them on the device (ps_order_masks_f32) -- nothing bigger than the orders crosses PCIe.
    order_on "device": the same integer work in one kernel on the masks where they are (csrc/ar_order.hip, bit for bit the host's
    results), the kernel masks queued behind it; what comes down for the host's wavefront schedules is the orders, the regions and
    the first sampled ranks.  Needs a mask on the device and a shape ps_plan_order_takes accepts: ValueError otherwise, no fallback.
    order_on None: the environment variable PS_PLAN_ORDER, "host" where it is not set.
    count_background: also keep every mask's number of set pixels (plan.background_counts), for PtsManipulator.forward_scene_step."""
    route = _order_route(order_on)
    if route == "device":
        return _build_ar_plan_device(background_mask, G, device, count_background)
    device = device or (background_mask.device if background_mask.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    B, S, _ = background_mask.shape
    L = G * G
    with _PLAN_LOCK:
        if background_mask.is_cuda:
            stage = _pinned("bg", (B, S, S), torch.uint8)
            as_u8 = (background_mask.view(torch.uint8) if background_mask.dtype == torch.bool and background_mask.is_contiguous()
                     else background_mask.to(torch.uint8))      # (a bool mask IS bytes of 0 / 1: no conversion pass in front of the copy)
            stage.copy_(as_u8, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            bg = stage.numpy()
        else:
            bg = background_mask.to(torch.uint8).contiguous().numpy()
        order_t, region_t = _pinned("order", (B, L), torch.int32), _pinned("region", (B, L), torch.uint8)
        order_loc, region = order_t.numpy(), region_t.numpy()
        _lib.call("ps_ar_plan", bg, B, S, G, order_loc, region, None, None, None, None)
        d_order, d_region = order_t.to(device, non_blocking=True), region_t.to(device, non_blocking=True)
        masks = [torch.empty(B, 9, L, dtype=torch.float32, device=device) for _ in range(3)]
        _lib.call("ps_order_masks_f32", d_order, B, G, G, *masks, _lib.status_word(device))
        plan = ARPlan(d_order, d_region, *masks, order_loc.copy(), region, (G, G))   # (the staging buffers are reused by the next plan)
        if count_background:   # set pixels per mask: what a batched chained scene's next frame adds to every cloud
            plan.background_counts = np.count_nonzero(np.asarray(bg).reshape(B, -1), axis=1).tolist()
        _finish_plan(plan, G, device)
    return plan


def _build_ar_plan_device(background_mask, G, device, count_background):
    """build_ar_plan(order_on="device"): ps_plan_order and ps_order_masks_f32 queued on the current stream, the orders, regions and first
    sampled ranks (5 KB per frame at G = 32) down through pinned buffers, one synchronisation, the schedules on the host as ever."""
    if not (isinstance(background_mask, torch.Tensor) and background_mask.is_cuda):
        raise ValueError("build_ar_plan(order_on='device') needs the background mask on the device (a CPU mask takes order_on='host')")
    if background_mask.dim() != 3 or background_mask.shape[1] != background_mask.shape[2]:
        raise ValueError(f"build_ar_plan: background_mask must be (B,S,S), got {tuple(background_mask.shape)}")
    B, S, _ = background_mask.shape
    if B < 1 or not _lib.call("ps_plan_order_takes", S, G):
        raise ValueError(f"build_ar_plan(order_on='device'): B = {B}, S = {S}, G = {G} is not a shape ps_plan_order takes")
    if device is not None and torch.device(device) != background_mask.device:
        raise ValueError(f"build_ar_plan(order_on='device'): the plan is built where the mask is ({background_mask.device}), not on {device}")
    device = background_mask.device
    L = G * G
    with _PLAN_LOCK, torch.cuda.device(device):
        as_u8 = (background_mask.view(torch.uint8) if background_mask.dtype == torch.bool and background_mask.is_contiguous()
                 else background_mask.to(torch.uint8).contiguous())
        d_order = torch.empty(B, L, dtype=torch.int32, device=device)
        d_region = torch.empty(B, L, dtype=torch.uint8, device=device)
        d_first = torch.empty(B, dtype=torch.int32, device=device)
        d_counts = torch.empty(B, dtype=torch.int32, device=device) if count_background else None
        _lib.call("ps_plan_order", as_u8, B, S, G, d_order, d_region, d_first, d_counts)
        masks = [torch.empty(B, 9, L, dtype=torch.float32, device=device) for _ in range(3)]
        _lib.call("ps_order_masks_f32", d_order, B, G, G, *masks, _lib.status_word(device))
        order_t, region_t = _pinned("order", (B, L), torch.int32), _pinned("region", (B, L), torch.uint8)
        first_t = _pinned("first_steps", (B,), torch.int32)
        order_t.copy_(d_order, non_blocking=True)
        region_t.copy_(d_region, non_blocking=True)
        first_t.copy_(d_first, non_blocking=True)
        if count_background:
            counts_t = _pinned("bg_counts", (B,), torch.int32)
            counts_t.copy_(d_counts, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        plan = ARPlan(d_order, d_region, *masks, order_t.numpy().copy(), region_t.numpy(), (G, G))
        if not np.array_equal(plan.first_steps, first_t.numpy()):   # (the kernel's first ranks against the ones its orders and regions give)
            raise RuntimeError("ps_plan_order: first_steps disagree with order_loc / region")
        if count_background:
            plan.background_counts = counts_t.numpy().tolist()
        _finish_plan(plan, G, device, first_steps_dev=d_first)
    return plan


def plan_from_reference_args(gen_order, masks, sample_region, device=None):
    """The ARPlan of values in the REFERENCE's form (what get_masks_for_batch returns without compact=True and what
    get_best_sample / sample() are handed, z_buffermodel.py:244-248): gen_order = list of (L,2) (row, col) arrays by rank,
    masks = (masks_init (b*513,9,L), masks_undilated (b*160,9,L), masks_dilated (b*80,9,L)) or their compact (b,9,L) forms,
    sample_region (b,H,W) = self.downsample(background_mask.float()): a block is sampled where it equals 1 (sample.py:24-41).
    Draws nothing from numpy's or torch's generators."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    B, (H, W) = len(gen_order), sample_region.shape[-2:]
    order_host = np.stack([np.asarray(g, np.int64)[:, 0] * W + np.asarray(g, np.int64)[:, 1] for g in gen_order]).astype(np.int32)
    region_host = (sample_region.detach().reshape(B, H * W).cpu().numpy() == 1).astype(np.uint8)
    m = [compact_mask(t.to(device), B, c).to(torch.float32) for t, c in zip(masks, (513, 160, 80))]
    m = [(t.expand(B, -1, -1) if t.size(0) == 1 and B > 1 else t).contiguous() for t in m]
    return ARPlan(torch.from_numpy(order_host).to(device), torch.from_numpy(region_host).to(device), *m, order_host, region_host, (H, W))
