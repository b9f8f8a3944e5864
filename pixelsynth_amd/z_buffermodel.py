"""View-synthesis orchestration of the hot path -- counterpart of the reference's
models/z_buffermodel.py:ZbufferModelPts for the rows of SURVEY.md 8(a): target poses
(get_rt_from_rot :202-242), reprojection + splat (forward_justpts), generation order + masks
(get_masks_for_batch :641-701), autoregressive outpainting (get_best_sample -> sample()) and the
foreground/background blend (get_combined :703-708).

The dense networks the reference runs around that path are SURVEY 8(f) "next" rows: the VQ-VAE-2 top level
(pixelsynth_amd/vqvae2), the depth Unet and the refinement decoder (pixelsynth_amd/networks) are built when the
options name them (`vqvae`, `norm_G` + `refine_model_type`) or can be injected (`pts_regressor`, `vqvae`,
`projector`); the discriminator / Places365 classifier of the sample ranking are injected only.  When a network is
absent the batch must carry the tensors it would have produced (`depths`, `codes`) -- that is how the synthetic
benchmark drives the hot path on its own.
"""
import math
import os
import types

import numpy as np
import torch
import torch.nn as nn

from .ar_plan import ARPlan, build_ar_plan, plan_from_reference_args
from .lmconv.layers import PONO
from .lmconv.model import TP_MIN_FRAMES, LaunchPipeline, OurPixelCNN, launch_capacity, wavefronts
from .lmconv.sample import sample
from .networks.f16x3 import checked
from .projection.z_buffer_manipulator import PtsManipulator

_PREFIX_STREAMS = {}    # (device, n) -> the prefix pass's side streams (ZbufferModelPts._prefix_streams)


def rank_samples(discrim_scores, entropy_scores):
    """Index of the sample get_best_sample keeps (z_buffermodel.py:266-276): samples are ranked by discriminator score
    (ascending) and by classifier entropy (ascending); total = .5*(n-1-entropy_rank) + .5*discrim_rank; the first
    arg-max wins.  Ranks come from numpy's default argsort, as there."""
    n = len(discrim_scores)
    by_disc, by_entr = np.argsort(np.asarray(discrim_scores)), np.argsort(np.asarray(entropy_scores))
    disc_rank, entr_rank = np.empty(n, np.int64), np.empty(n, np.int64)
    disc_rank[by_disc] = np.arange(n)
    entr_rank[by_entr] = np.arange(n)
    return int(np.argmax(.5 * (n - 1 - entr_rank) + .5 * disc_rank))


RANK_ROUTES = ("host", "device")


def _rank_route(rank_on, opt):
    """rank_on of get_best_sample -> "host" / "device"; None: opt.rank_on, then the environment variable PS_RANK (read per call), host
    by default"""
    route = rank_on if rank_on is not None else getattr(opt, "rank_on", None)
    if route is None:
        route = os.environ.get("PS_RANK", "host")
    if route not in RANK_ROUTES:
        raise ValueError(f"get_best_sample: rank_on / opt.rank_on / PS_RANK is {route!r}, expected one of {RANK_ROUTES}")
    return route


RANK_SCOPES = ("batch", "view")


def _rank_scope(rank_scope, opt):
    """rank_scope of get_best_sample -> "batch" (one winner index for the whole batch: the reference's rule) / "view" (the best
    candidate of every view); None: opt.rank_scope, then the environment variable PS_RANK_SCOPE (read per call), batch by default"""
    scope = rank_scope if rank_scope is not None else getattr(opt, "rank_scope", None)
    if scope is None:
        scope = os.environ.get("PS_RANK_SCOPE", "batch")
    if scope not in RANK_SCOPES:
        raise ValueError(f"get_best_sample: rank_scope / opt.rank_scope / PS_RANK_SCOPE is {scope!r}, expected one of {RANK_SCOPES}")
    return scope


def view_draws(n, B, L):
    """(n, B, L) uniforms on the host for n candidates of B views: entry [i, b] is the (1, L) draw of manual_seed(i) for every b -- a
    view gets the draws of a B = 1 run, never row b of a (B, L) draw: it is the same picture alone or in a batch"""
    return torch.stack([torch.rand(1, L, generator=torch.Generator(device="cpu").manual_seed(i)).expand(B, L) for i in range(n)])


class _SceneState:
    """What forward_scene carries from one rendered frame to the next (z_buffermodel.py:436-443)."""

    def __init__(self, img):
        self.img = img                # the frame the next one is rendered from
        self.cloud = None             # (1,4,N) every point so far, in the camera of the last rendered frame
        self.feats = None             # (1,C,N) their features
        self.background = None        # (1,S,S) background mask of the last rendered frame
        self.out_RTinv = None         # inverse pose of the last rendered frame
        self.numerator = None
        self.direction = None
        self.scenes = None            # B > 1: the projection.SceneState of the batch (ragged clouds kept on the device) in place of
        self.new_counts = None        # cloud / feats, and the set pixels of every scene's `background` where the AR plan counted them


class _PipeBuffers:
    """What outpaint_pipelined keeps between calls.  The batches in flight live in ONE engine handle of depth x V frames: batch i in
    frames [V slot, ...), its slot dealt by `sched` (lmconv.model.LaunchPipeline, the host side).  The per-frame arrays of the C ABI
    (codes, order, region, the three masks, uniforms) are persistent (depth x V, ...) tensors; a batch's plan is copied into its share
    on the stream of the AR run (14 MB, ~10 us), so that planning on a side stream never writes under a launch that still reads another
    batch's share."""

    def __init__(self, V, depth, L, device):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        F_ = depth * V
        self.V, self.device, self.sched = V, device, LaunchPipeline(depth)
        self.codes, self.order, self.region = z((F_, L), torch.int32), z((F_, L), torch.int32), z((F_, L), torch.uint8)
        self.masks = [z((F_, 9, L), torch.float32) for _ in range(3)]
        self.uniforms, self.first_steps = z((F_, L), torch.float32), z((F_,), torch.int32)
        self.offset = [torch.tensor([k * V, 0], dtype=torch.int32, device=device) for k in range(depth)]   # a slot's frame offset
        self.order[:] = torch.arange(L, device=device, dtype=torch.int32)   # (a frame nobody has planned yet still holds a permutation)
        self.args = (self.codes, self.order, self.region, *self.masks)


class ZbufferModelPts(nn.Module):
    def __init__(self, opt, pts_regressor=None, vqvae=None, projector=None, encoder=None, classifier=None):
        super().__init__()
        self.opt = opt
        if pts_regressor is None and hasattr(opt, "norm_G"):  # z_buffermodel.py:41-44
            from .networks import Unet
            extra = {"num_filters": opt.Unet_num_filters} if hasattr(opt, "Unet_num_filters") else {}
            pts_regressor = Unet(channels_in=3, channels_out=1, opt=opt, **extra)
        if projector is None and "resnet" in getattr(opt, "refine_model_type", "") and hasattr(opt, "norm_G"):  # :90
            from .networks import get_decoder
            projector = get_decoder(opt)
        self.pts_regressor = pts_regressor
        self.encoder = encoder        # feature encoder when use_rgb_features is off (injected)
        if classifier is None and max(int(getattr(opt, "num_samples", 1)), 1) > 1:   # z_buffermodel.py:88 (random init until the
            from .networks import resnet18                                             # Places365 state_dict is loaded, demo.py:233-243)
            classifier = resnet18(num_classes=365)
        self.classifier = classifier  # Places365 ResNet-18 of get_best_sample
        if vqvae is None and getattr(opt, "vqvae", False):  # z_buffermodel.py:81-82
            from .vqvae2 import VQVAETop
            vqvae = VQVAETop()
        self.vqvae = vqvae
        self.projector = projector
        C = 3 if getattr(opt, "use_rgb_features", True) else 64
        self.pts_transformer = PtsManipulator(opt.W, C=C, opt=opt)
        self.num_classes = 512
        self.outpaint2 = OurPixelCNN(nr_resnet=2, nr_filters=80, input_channels=self.num_classes,
                                     nr_logistic_mix=10, kernel_size=(3, 3), max_dilation=2, weight_norm=False,
                                     feature_norm_op=lambda c: PONO(), dropout_prob=0, conv_bias=True,
                                     conv_mask_weight=False, rematerialize=False, binarize=False)  # :62-74
        self.args = types.SimpleNamespace(dataloader_seed=getattr(opt, "seed", 0), num_classes=self.num_classes)
        self.obs = [3, 32, 32]
        self.downsample = nn.AvgPool2d(kernel_size=8, stride=8)
        self.rotvecs = {'R': np.array([0, .6, 0]), 'L': np.array([0, -.6, 0]), 'U': np.array([-.3, 0, 0]),
                        'D': np.array([.3, 0, 0]), 'UR': np.array([-.15, .3, 0]), 'UL': np.array([-.15, -.3, 0]),
                        'DR': np.array([.15, .3, 0]), 'DL': np.array([.15, -.3, 0])}  # :113-114
        self.mapping = ['R', 'L', 'U', 'D', 'UL', 'UR', 'DR', 'DL']
        self.sample_batch = 32        # frames (candidates x views) a get_best_sample engine run takes at most

    # ---------------------------------------------------------------- a15
    def eulerAnglesToRotationMatrix(self, theta):
        """z_buffermodel.py:186-200."""
        R_x = np.array([[1, 0, 0], [0, math.cos(theta[0]), -math.sin(theta[0])],
                        [0, math.sin(theta[0]), math.cos(theta[0])]])
        R_y = np.array([[math.cos(theta[1]), 0, math.sin(theta[1])], [0, 1, 0],
                        [-math.sin(theta[1]), 0, math.cos(theta[1])]])
        R_z = np.array([[math.cos(theta[2]), -math.sin(theta[2]), 0],
                        [math.sin(theta[2]), math.cos(theta[2]), 0], [0, 0, 1]])
        return np.dot(R_z, np.dot(R_y, R_x))

    def get_rt_from_rot(self, direction, input_RT, num=None, denom=None):
        """z_buffermodel.py:202-242 -> (new_output_RTinv, new_output_RT), same device as input_RT."""
        dev = input_RT.device
        if num is None:
            num = 0
        setting = getattr(self.opt, "model_setting", "gen_img")
        if setting in ('gen_two_imgs', 'gen_scene'):
            if direction == 'S':
                new_RT = torch.zeros_like(input_RT)
                new_RT[:, :, :3] = input_RT[:, :, :3]
                new_RT[:, 3, 3] = 1
                off = torch.tensor([np.sin(2 * np.pi * num / denom), np.cos(2 * np.pi * num / denom),
                                    .4 * np.sin(2 * np.pi * (.25 + num / denom))]).to(dev)
                new_RT[0, :3, 3] = input_RT[0, :3, 3] + .35 * off
                return torch.inverse(new_RT), new_RT
            elif direction == 'C':
                rotvec = np.array([0.2 * np.cos(2 * np.pi * num / denom), 0.2 * np.sin(2 * np.pi * num / denom), 0])
            else:
                rotvec = self.rotvecs[direction] * num / denom
        else:
            rotvec = self.rotvecs[direction] * self.opt.rotation / np.linalg.norm(self.rotvecs[direction])
        mtx = torch.zeros([1, 4, 4], device=dev)
        mtx[0, 3, 3] = 1
        mtx[0, :3, :3] = torch.tensor(self.eulerAnglesToRotationMatrix(rotvec)).to(torch.float32).to(dev)
        if getattr(self.opt, "homography", False) and direction not in ('C',):
            new_RT = torch.zeros([1, 4, 4], device=dev)
            new_RT[:, :, 3] = input_RT[:, :, 3]
            new_RT[:, :3, :3] = mtx[:, :3, :3].bmm(input_RT[:, :3, :3])
        else:
            new_RT = mtx.bmm(input_RT)
        return torch.inverse(new_RT), new_RT

    # ---------------------------------------------------------------- depth of the source image (forward_image :303-311, :606-612)
    def regress_depth(self, input_img, given=None):
        """The reference's depth rule, ONE place for every entry point: the regressor's sigmoid scaled to [min_z, max_z], or
        1 / (10 sigmoid + 0.01) with opt.use_inverse_depth (landscape datasets), or the given depth with opt.use_gt_depth --
        and `given` stands in for the regressor when the model has none (the synthetic benchmark)."""
        if self.pts_regressor is None or getattr(self.opt, "use_gt_depth", False):
            if given is None:
                raise ValueError("no depth regressor (or opt.use_gt_depth): the batch must carry the depth")
            return given
        raw = torch.sigmoid(self.pts_regressor(input_img))
        if getattr(self.opt, "use_inverse_depth", False):
            return 1. / (raw * 10 + 0.01)
        return raw * (self.opt.max_z - self.opt.min_z) + self.opt.min_z

    # ---------------------------------------------------------------- a7
    def get_masks_for_batch(self, output_RT, input_RTinv, background_mask, compact=False):
        """z_buffermodel.py:641-701.  Default return value matches the reference: masks repeated per input
        channel, (b*513,9,L), (b*160,9,L), (b*80,9,L), plus gen_order (list of (L,2) arrays).
        compact=True returns the ARPlan the HIP sampler consumes directly (one (b,9,L) copy per mask)."""
        plan = build_ar_plan(background_mask, self.obs[1])
        if compact:
            return plan
        b, L = plan.mask_init.shape[0], self.obs[1] * self.obs[2]
        rep = lambda m, c: m.unsqueeze(1).repeat(1, c, 1, 1).view(-1, 9, L)
        return rep(plan.mask_init, 513), rep(plan.mask_undilated, 160), rep(plan.mask_dilated, 80), plan.gen_order

    # ---------------------------------------------------------------- a14
    def get_combined(self, gen_fs, ar_sample, background_mask):
        """z_buffermodel.py:703-708."""
        b, h, w = background_mask.shape
        foreground_mask = (~background_mask).float()
        background_mask = background_mask.float()
        return gen_fs * foreground_mask.view(b, -1, h, w) + ar_sample * background_mask.view(b, -1, h, w)

    # ---------------------------------------------------------------- batched hot path (C3/C4/C5)
    @torch.no_grad()
    def plan_views(self, fs, depth, K, K_inv, input_RT, input_RTinv, output_RT, output_RTinv):
        """First half of outpaint_views: reproject + splat (a2-a6) on the current stream, then the host part -- the
        background masks come back, generation orders, kernel masks and the wavefront schedule are built (a7-a9) and
        uploaded.  Ends with everything the AR run needs resident on the device.
        -> dict(gen_fs, background_mask, plan)."""
        gen_fs, background_mask = self.pts_transformer.forward_justpts(fs, depth, K, K_inv, input_RT, input_RTinv,
                                                                      output_RT, output_RTinv)
        return dict(gen_fs=gen_fs, background_mask=background_mask, plan=build_ar_plan(background_mask, self.obs[1]))

    @staticmethod
    def adopt_planned(planned, stream):
        """A plan made on a side stream is about to be consumed on `stream`: tell the caching allocator, so that the
        plan's buffers are not recycled on the side stream while work queued on `stream` still reads them."""
        for t in [planned["gen_fs"], planned["background_mask"]] + planned["plan"].device_tensors():
            if t.numel():
                t.record_stream(stream)

    @torch.no_grad()
    def outpaint_planned(self, planned, codes, temperature=0.7, uniforms=None, forced=None, between=None):
        """Second half: AR outpainting of the 32x32 code grids (a13) of the views prepared by plan_views; asynchronous
        on the current stream.  Adds `codes` (V,32,32) int32 to the dict and returns it.
        between: a callable run on the current stream BETWEEN the whole-grid prefix pass and the first column launch (the two
        halves of the AR run, ps_pixelcnn_ar_prefix / ps_pixelcnn_ar_columns).  bench.py makes the stream wait there
        for the previous step's asynchronous frame gather: the collective's kernels then run beside the prefix pass -- whose
        small workgroups fit around them -- and are through before a column launch asks for every compute unit."""
        gen_fs, plan = planned["gen_fs"], planned["plan"]
        V = gen_fs.shape[0]
        L = self.obs[1] * self.obs[2]
        if codes is None:  # z_buffermodel.py:345: the VQ-VAE top codes of the reprojected view
            codes = self.vqvae.encode_codes(gen_fs)
        c32 = codes.reshape(V, L).to(torch.int32).contiguous().clone()
        eng = self.outpaint2.engine(self.obs[1], self.obs[2], V)
        if forced is None and uniforms is None:
            uniforms = torch.rand(V, L, device=gen_fs.device, dtype=torch.float32)
        nsplit = self._prefix_split(V, busy=between is not None)
        # per-frame prefixes where the plan carries their schedule (build_ar_plan): the whole-grid pass takes every frame up to ITS first
        # sampled position, the columns start there (ps_pixelcnn_ar_prefix_frames / ps_ar_wavefronts_frames: the same codes)
        # (batches of the throughput form only: the launches of a small batch are bound by their latency, not by their columns --
        # 16 views: 5.55 ms per step with one prefix for the batch, 5.66 with per-frame ones)
        waves, pf = plan.schedule(self.PER_FRAME_PREFIX and V >= TP_MIN_FRAMES)
        args = (c32, plan.order_loc, plan.region, plan.mask_init, plan.mask_undilated, plan.mask_dilated)
        if (between is None and nsplit == 1 and not pf) or plan.first_step >= L:   # (nothing to walk: only the whole-grid pass runs)
            eng.ar_run(*args, temperature=temperature, uniforms=uniforms, forced=forced, first_step=plan.first_step, waves=waves)
            if between is not None:
                between()
        else:
            self._prefix_pass(eng, args, plan.first_step, 0, V, nsplit, pf, record=True)
            if between is not None:
                between()
            eng.ar_columns(*args, waves, temperature=temperature, uniforms=uniforms, forced=forced, first_step=plan.first_step)
        planned["codes"] = c32.view(V, self.obs[1], self.obs[2])
        return planned

    def _prefix_pass(self, eng, args, first_step, lo, hi, nsplit, pf, record=False):
        """The whole-grid prefix pass of frames [lo, hi) of `args` (codes, order, region, the three masks), dealt to nsplit ranges
        (_prefix_split): the first on the current stream, the others each on a side stream of their own (_prefix_streams), which the
        current stream then waits for.  ps_pixelcnn_ar_prefix is built for it -- every range has its part of the scratch: a launch
        empties over its last tenth, and the next stage's launch cannot start before it has -- with a second range's launches in
        flight, their workgroups take the places as they fall free.  record: the tensors are the caller's own (outpaint_planned's
        are per batch), so the caching allocator is told that the side streams read them."""
        if nsplit == 1:
            eng.ar_prefix(*args, first_step, frame_begin=lo, frame_end=hi, **pf)
            return
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(main)
        per = (hi - lo) // nsplit
        sides = self._prefix_streams(nsplit - 1, args[0].device)
        for k, side in enumerate(sides):
            side.wait_event(ready)
            with torch.cuda.stream(side):
                eng.ar_prefix(*args, first_step, frame_begin=lo + (k + 1) * per, frame_end=lo + (k + 2) * per if k + 2 < nsplit else hi, **pf)
            if record:
                for t in args + ((pf["first_steps"],) if pf else ()):
                    t.record_stream(side)
        eng.ar_prefix(*args, first_step, frame_begin=lo, frame_end=lo + per, **pf)
        for side in sides:
            main.wait_stream(side)

    # ---------------------------------------------------------------- the AR runs of consecutive batches, overlapped
    PIPE_CAP = 1024         # columns a merged launch takes (lmconv.model.COLUMNS_PER_LAUNCH_TP)
    PER_FRAME_PREFIX = True  # outpaint_pipelined: per-frame prefixes where the plan carries their schedule (build_ar_plan, PS_PER_FRAME_PREFIX)
    PIPE_DEPTH = 4          # batches outpaint_pipelined keeps in flight at least (pipe_depth): every launch takes what is left of each batch's
    #                         current wavefront, oldest batch first, while there is room (lmconv.model.pack_launches) -- with three to four in
    #                         flight the launches of a large batch are full (C5's 128 views: 33 launches of ~1 020 columns per step
    #                         where head / tail merging ran 45 of 750; 16 views: 33 of 128 where equal parts ran 44)
    PIPE_FRAMES = 384       # ... and as many as it takes to have about this many frames in the handle, eight at most: the throughput form's
    #                         launches take 1 024 columns, which middle-sized batches only fill with more of them in flight (ms per step with
    #                         4 / 6 / 8 in flight -- 24 views: 5.08 / 4.39 / 4.10, 32: 5.21 / 4.53 / 4.36, 48: 6.23 / 5.80 / 5.73, 64: 6.82 / 6.48,
    #                         96: 9.04 / 8.93; 128: the same from 4 on; 16, latency form: 3.38 / 3.41 / 3.52)

    def pipe_depth(self, V):
        """Batches of V views that outpaint_pipelined keeps in flight at most (PS_PIPE_DEPTH overrides): the frames of its engine handle
        are that many batches'; a batch's result comes back at most depth - 1 calls late."""
        d = os.environ.get("PS_PIPE_DEPTH")
        if d:
            return max(2, min(8, int(d)))
        if V < TP_MIN_FRAMES:        # (latency form: launches of 128 columns, full at four)
            return self.PIPE_DEPTH
        return max(self.PIPE_DEPTH, min(8, int(round(self.PIPE_FRAMES / V))))

    def pipe_frames(self, V):
        """Frames of the engine handle outpaint_pipelined runs batches of V views in."""
        return self.pipe_depth(V) * V

    def _pipe_buffers(self, V, device):
        """The pipeline of batches of V views (_PipeBuffers), made anew when V, the device or the depth has changed."""
        st = self.__dict__.get("_pipe")
        D = self.pipe_depth(V)
        if st is not None and (st.V != V or st.device != device or st.sched.depth != D):
            if st.sched.inflight or st.sched.done:
                raise RuntimeError("outpaint_pipelined: a batch of another size is still in flight (call outpaint_flush first)")
            st = None
        if st is None:
            st = self.__dict__["_pipe"] = _PipeBuffers(V, D, self.obs[1] * self.obs[2], device)
        return st

    @torch.no_grad()
    def outpaint_pipelined(self, planned, codes, temperature=0.7, uniforms=None, between=None):
        """outpaint_planned for callers with a STREAM of batches of V views (bench.py, driver.py).  A batch's wavefronts grow to the
        launch capacity and shrink to a handful of columns, and a launch costs its 33 dependent stages whatever it holds: up to
        pipe_depth(V) batches are resident in ONE engine handle of pipe_frames(V) frames, and every column launch takes what is left of
        each batch's current wavefront, oldest batch first, while there is room (lmconv.model.pack_launches) -- C5's 128 views: 33
        launches of ~1 020 columns per step instead of 45 of 750 (head / tail merging of two batches, round 5) or 91 of a batch alone.
        Every column still runs behind the columns it reads (a batch moves on to its next wavefront only in the launch after the one
        that took the last of the current one), so the codes are outpaint_planned's, bit for bit (tests/test_zbuffermodel_gpu.py,
        tests/test_config_size_gpu.py).  Asynchronous on the current stream.
        -> the dict (codes added) of the next batch, in submission order, that is complete -- at most pipe_depth(V) - 1 calls late -- or
        None; outpaint_flush() runs what is left.  between: as for outpaint_planned."""
        gen_fs, plan = planned["gen_fs"], planned["plan"]
        V, G = gen_fs.shape[0], self.obs[1]
        L = G * self.obs[2]
        st = self._pipe_buffers(V, gen_fs.device)
        if codes is None:
            codes = self.vqvae.encode_codes(gen_fs)
        if uniforms is None:
            uniforms = torch.rand(V, L, device=gen_fs.device, dtype=torch.float32)
        eng = self.outpaint2.engine(G, self.obs[2], st.sched.depth * V)
        if st.sched.inflight and st.sched.inflight[0]["temperature"] != temperature:
            # what is in flight was planned with ANOTHER temperature: it cannot ride in this batch's launches (a launch has one
            # temperature), so it is finished now, as launches of its own, with its own -- the codes stay those of outpaint_planned
            self._pipe_step(eng, st, drain=True)
        h = st.sched.free_slot()
        lo, hi = h * V, (h + 1) * V
        # (as elementwise kernels, not Tensor.copy_: same-type copies go through hipMemcpyAsync, which on the stream of the AR run stalled
        # for ~60 ms every few steps)
        put = lambda dst, src: torch.add(src, 0, out=dst) if src.dtype == dst.dtype else dst.copy_(src)
        put(st.codes[lo:hi], codes.reshape(V, L))
        put(st.order[lo:hi], plan.order_loc)
        put(st.region[lo:hi], plan.region)
        for dst, src in zip(st.masks, (plan.mask_init, plan.mask_undilated, plan.mask_dilated)):
            put(dst[lo:hi], src.expand(V, -1, -1) if src.size(0) == 1 else src)
        put(st.uniforms[lo:hi], uniforms)
        # PER-FRAME prefixes (plans that carry their schedule): the whole-grid pass takes every frame up to ITS first sampled position --
        # a location costs it half of what a column costs, and the bits are the same
        waves, pf = plan.schedule(self.PER_FRAME_PREFIX)
        if pf:
            put(st.first_steps[lo:hi], pf["first_steps"])
            pf["first_steps"] = st.first_steps
        # the prefix pass of this batch's frames (two ranges on two streams, as in outpaint_planned)
        self._prefix_pass(eng, st.args, plan.first_step, lo, hi, self._prefix_split(V, busy=between is not None), pf)
        if between is not None:
            between()
        # this batch's schedule, in the handle's frame numbering, joins the batches in flight.  The columns are on the device already (the
        # plan's upload); a call's launches are put together THERE, from slices of the batches' columns (one concatenation) -- nothing
        # crosses PCIe on the stream of the AR run.
        st.sched.admit(np.asarray(waves[1]), plan.first_step, temperature, planned=planned, slot=h,
                       cols=waves[0] + st.offset[h] if h else waves[0])
        self._pipe_step(eng, st)
        done = st.sched.pop()
        return None if done is None else done["planned"]

    def _pipe_step(self, eng, st, drain=False):
        """One call's launches out of the batches in flight (lmconv.model.LaunchPipeline.step), each group of them put together from
        slices of the batches' columns; batches whose last column has been queued are complete: their codes are taken out of the handle
        behind the launches."""
        cap = min(int(os.environ.get("PS_PIPE_CAP", self.PIPE_CAP)), self.PIPE_CAP, launch_capacity(st.V))
        for group, starts, first, temperature, finished in st.sched.step(cap, drain):
            if group:
                self._pipe_columns(eng, st, torch.cat([b["cols"][a:e] for b, a, e in group]), starts, first, temperature)
            for b in finished:
                lo = b["slot"] * st.V
                b["planned"]["codes"] = st.codes[lo:lo + st.V].clone().view(st.V, self.obs[1], self.obs[2])

    def _pipe_columns(self, eng, st, cols, ws, first, temperature):
        if len(ws) > 1 and ws[-1] > 0:
            eng.ar_columns(*st.args, (cols.contiguous(), np.ascontiguousarray(ws, np.int32)), temperature=temperature, uniforms=st.uniforms,
                           first_step=int(first))

    @torch.no_grad()
    def outpaint_flush(self):
        """What outpaint_pipelined still holds: the remaining parts of the batches in flight, as launches of their own
        -> the dicts of the batches not handed back yet, oldest first ([] when there is none)."""
        st = self.__dict__.get("_pipe")
        if st is None:
            return []
        if st.sched.inflight:
            self._pipe_step(self.outpaint2.engine(self.obs[1], self.obs[2], st.sched.depth * st.V), st, drain=True)
        return [b["planned"] for b in st.sched.flush()]

    def outpaint_reset(self):
        """Forget the batches outpaint_pipelined still holds (their remaining wavefronts never run; their codes are lost).  For a caller
        whose sequence of batches was cut short by an exception: without this the NEXT sequence of the same batch size would merge the
        stale batches into its first launches and get their dicts back as its first results (driver.render_pipelined and bench.py call
        it on their way out of a failed run)."""
        st = self.__dict__.get("_pipe")
        if st is not None:
            st.sched.reset()

    PREFIX_SPLIT_MIN_VIEWS = 64   # below this a launch of half the frames no longer fills the chip
    PREFIX_STREAMS = 2            # 128 views: 18.16 -> 17.95 ms per step (three alternating pairs); 4 ranges lose (18.59)

    def _prefix_split(self, V, busy=False):
        """Frame ranges the prefix pass of a V-view batch is dealt to (each on a stream of its own): PREFIX_STREAMS, or
        PS_PREFIX_STREAMS from the environment; 1 for batches too small to fill the chip twice over or not a multiple of 8 frames
        per range (a range's frames are dealt to the 8 XCDs).  busy: collectives are in flight beside the AR run (the caller passed
        between=) -- with the runtime's default of four hardware queues one more stream then shares a queue with another and the step
        gets SLOWER (19.5 against 18.4 ms), so the pass is split only when the process runs with GPU_MAX_HW_QUEUES >= 8 (18.1 ms;
        bench.py sets it, tools/hwq_ab.sh measured it)."""
        n = int(os.environ.get("PS_PREFIX_STREAMS", self.PREFIX_STREAMS))
        if busy and "PS_PREFIX_STREAMS" not in os.environ and int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 8:
            n = 1
        return n if n > 1 and V >= self.PREFIX_SPLIT_MIN_VIEWS and V % (8 * n) == 0 else 1

    def _prefix_streams(self, n, device):
        """n side streams for the prefix pass, created once per PROCESS and device: which hardware queue a stream lands on is dealt at
        creation, one in eight shares the main stream's (docs/LAB_NOTEBOOK.md, "Which stream the side stream is") -- a process that
        builds several models one after the other (bench.py's side configurations) must not draw a new lot with each of them
        (round 6: C4's 64-frame circle 8.8 ms per step inside the long default bench run, 6.9 as a run of its own)."""
        key = (str(device), n)
        cache = _PREFIX_STREAMS
        if key not in cache:
            skip = int(os.environ.get("PS_PREFIX_STREAM_SKIP", "0"))    # tuning: streams created (and kept) in front of them
            cache[("skip",) + key] = [torch.cuda.Stream(device=device) for _ in range(skip)]
            cache[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
        return cache[key]

    def outpaint_views(self, fs, depth, K, K_inv, input_RT, input_RTinv, output_RT, output_RTinv, codes,
                       temperature=0.7, uniforms=None, forced=None, check=True):
        """V independent novel views in one pass: reproject + splat (a2-a6), order + masks (a7-a9),
        AR outpainting of the 32x32 code grid (a13, fused device loop).
        fs (V,C,S,S), depth (V,1,S,S), cameras (V,4,4), codes (V,32,32) int (the VQ-VAE codes of the
        reprojected view; synthetic in the benchmark).  Returns dict(gen_fs, background_mask, codes, plan).
        Callers with several batches can overlap the host part of the next batch with the AR run of this one:
        plan_views on a side stream while outpaint_planned runs (bench.py, driver.py do)."""
        planned = self.plan_views(fs, depth, K, K_inv, input_RT, input_RTinv, output_RT, output_RTinv)
        out = self.outpaint_planned(planned, codes, temperature, uniforms, forced)
        if check:   # synchronises; pipelined callers (plan_views / outpaint_planned) pass check=False and ask the engine once
            self.outpaint2.engine(self.obs[1], self.obs[2], fs.shape[0]).check()
        return out

    @torch.no_grad()
    def synthesize_views(self, src_imgs, view_src, K, K_inv, input_RT, input_RTinv, output_RT, output_RTinv, temperature=None,
                         uniforms=None, depths=None, check=True):
        """END TO END for V independent (source, target view) pairs in one pass -- the batched counterpart of forward_image
        (z_buffermodel.py:291-419, num_samples = 1): depth Unet on the n_src SOURCE images (once per source, not per view),
        reproject + splat, VQ-VAE top codes of the reprojected views, AR outpainting, decode_code, get_combined, refinement
        decoder.  src_imgs (n_src,3,S,S); view_src (V,) long: the source of every view; cameras / poses (V,4,4);
        depths (n_src,1,S,S) stands in for the regressor when the model has none.
        -> dict(PredImg (V,3,S,S), FeaturesImg, background_mask, codes, depth)."""
        depth_src = self.regress_depth(src_imgs, depths)   # :303-311
        fs_src = src_imgs if getattr(self.opt, "use_rgb_features", True) else self.encoder(src_imgs)
        planned = self.plan_views(fs_src[view_src].contiguous(), depth_src[view_src].contiguous(), K, K_inv, input_RT, input_RTinv,
                                  output_RT, output_RTinv)
        out = self.outpaint_planned(planned, None, self.opt.temperature if temperature is None else temperature, uniforms)
        if check:
            self.outpaint2.engine(self.obs[1], self.obs[2], K.shape[0]).check()
        pred = self._decode_checked(out["gen_fs"], out["background_mask"], out["codes"], check)
        return dict(PredImg=pred, FeaturesImg=out["gen_fs"], background_mask=out["background_mask"], codes=out["codes"],
                    depth=depth_src, plan=out["plan"])

    # ---------------------------------------------------------------- reference-shaped single image path
    @torch.no_grad()
    def forward_image(self, batch, netD=None, rank_on=None):
        """Hot-path part of forward_image (z_buffermodel.py:291-419) for model_setting gen_img / gen_paired_img.
        batch: {"images": [(B,3,S,S)], "cameras": [{"P","Pinv","K","Kinv"}], optional "depths": [(B,1,S,S)],
        optional "codes": (B,32,32)} -> (None, outputs dict with the reference's keys).  rank_on: get_best_sample's."""
        dev = next(self.parameters()).device   # (the renderer itself refuses anything but the GPU)
        input_img = batch["images"][0].to(dev)
        cam = {k: v.to(dev) for k, v in batch["cameras"][0].items() if torch.is_tensor(v)}
        K, K_inv, input_RT, input_RTinv = cam["K"], cam["Kinv"], cam["P"], cam["Pinv"]
        paired = getattr(self.opt, "model_setting", "gen_img") == "gen_paired_img"
        if paired:   # :294-295 (process_batch :127-130): the target view comes with the batch
            output_img = batch["images"][-1].to(dev)
            output_RT, output_RTinv = batch["cameras"][-1]["P"].to(dev), batch["cameras"][-1]["Pinv"].to(dev)
        else:
            output_RTinv, output_RT = self.get_rt_from_rot(self.opt.direction, input_RT)
        regressed_pts = self.regress_depth(input_img, batch["depths"][0].to(dev) if "depths" in batch else None)   # :303-311
        fs = input_img if getattr(self.opt, "use_rgb_features", True) else self.encoder(input_img)
        gen_fs, background_mask = self.pts_transformer.forward_justpts(fs, regressed_pts, K, K_inv, input_RT,
                                                                      input_RTinv, output_RT, output_RTinv)
        outputs = {"InputImg": input_img, "PredDepthImg": regressed_pts / 5 - 1,
                   "ForegroundImg": (~background_mask).repeat(input_img.shape[0], 1, 1, 1).float(), "FeaturesImg": gen_fs}
        if paired:
            outputs["OutputImg"] = output_img
        if getattr(self.opt, "no_outpainting", False):   # :383-384
            outputs["PredImg"] = self._project_checked(gen_fs, None)
            return None, outputs
        if self.vqvae is not None:
            enc = getattr(self.vqvae, "encode_codes", None)      # our mirror: top codes only, int32, on the device
            downsampled_fs = enc(gen_fs) if enc is not None else self.vqvae.encode(gen_fs)[3]
        else:
            downsampled_fs = batch["codes"].to(dev)
        if max(int(getattr(self.opt, "num_samples", 1)), 1) > 1:   # :349 -> get_best_sample with opt.num_samples candidates
            plan = self.get_masks_for_batch(output_RT, input_RTinv, background_mask, compact=True)
            outputs["PredImg"] = self.get_best_sample(plan, downsampled_fs, background_mask, gen_fs, netD, input_img,
                                                      shard=bool(getattr(self.opt, "shard_samples", False)), rank_on=rank_on,
                                                      rank_scope=getattr(self.opt, "rank_scope", None))
            return None, outputs
        masks_init, masks_undilated, masks_dilated, gen_order = self.get_masks_for_batch(output_RT, input_RTinv,
                                                                                         background_mask)
        autoreg_output, _ = sample(self.outpaint2, gen_order, masks_init, masks_undilated, masks_dilated,
                                   downsampled_fs, self.obs, self.args, 0, self.opt.temperature,
                                   self.downsample(background_mask.float()))
        codes = torch.argmax(autoreg_output, dim=1)
        outputs["PredCodes"] = codes
        if self.vqvae is not None:  # :250-252 (without a refinement net the blend itself is the prediction)
            outputs["PredImg"] = self._decode_checked(gen_fs, background_mask, codes.to(torch.int64))
        return None, outputs

    # ---------------------------------------------------------------- the likelihood of given codes (z_buffermodel.py:351-381, :398)
    @torch.no_grad()
    def autoreg_score(self, plan_or_masks, target_codes, temperature=1.0):
        """The likelihood the PixelCNN gives to target_codes (B,32,32) in the generation order of plan_or_masks (the compact ARPlan, or
        the three masks as get_masks_for_batch returns them) -> likelihood.CodeNLL: likelihood.score_codes, the method form."""
        from .likelihood import score_codes
        return score_codes(self, target_codes.reshape(-1, self.obs[1], self.obs[2]), plan_or_masks, temperature=temperature)

    @torch.no_grad()
    def forward_validation(self, batch):
        """The reference's TEACHER-FORCED forward (z_buffermodel.py:351-381, the 'train' branch of forward_image) without gradients, for
        a batch that carries the target view as gen_paired_img batches do: images [source, ..., target], cameras [source, ..., target],
        optional "depths", and "codes" (B,32,32) -- the target's codes -- when the model has no VQ-VAE.  Depth, reprojection + splat and
        the generation order as forward_image; the target's codes (vqvae.encode_codes(target)) are scored under the PixelCNN in that
        order (autoreg_score: :358-362), and the decoder sees the reprojected features where visible and the decoded TARGET codes in
        the background, as a stand-in for the AR output (:372-380).  opt.model_setting is not read.
        -> (loss, outputs).  outputs: the keys of forward_image -- PredImg is the teacher-forced prediction (with a VQ-VAE), OutputImg
        the target -- and NLLMap, EntropyMap (B,1,32,32), nats at T = 1, PredCodes the target's codes.  loss, 0-dim fp64 device
        tensors: autoreg_loss, the mean nats over all B * 1024 locations at T = 1 -- what nn.CrossEntropyLoss() returns at :362 --,
        ar_bits_per_code, ar_bits_sampled, ar_bits_observed (/ ln 2; NaN for a group without a location), ar_accuracy_sampled; and
        ar_frames, the (B,2,4) fp64 table of likelihood.CodeNLL.frames, for callers that report per pair."""
        if len(batch["images"]) < 2 or len(batch["cameras"]) < 2:
            raise ValueError("forward_validation: the batch carries the target view, images [source, target] and cameras [source, target]")
        dev = next(self.parameters()).device
        input_img, output_img = batch["images"][0].to(dev), batch["images"][-1].to(dev)
        cam = {k: v.to(dev) for k, v in batch["cameras"][0].items() if torch.is_tensor(v)}
        K, K_inv, input_RT, input_RTinv = cam["K"], cam["Kinv"], cam["P"], cam["Pinv"]
        output_RT, output_RTinv = batch["cameras"][-1]["P"].to(dev), batch["cameras"][-1]["Pinv"].to(dev)
        regressed_pts = self.regress_depth(input_img, batch["depths"][0].to(dev) if "depths" in batch else None)
        fs = input_img if getattr(self.opt, "use_rgb_features", True) else self.encoder(input_img)
        gen_fs, background_mask = self.pts_transformer.forward_justpts(fs, regressed_pts, K, K_inv, input_RT, input_RTinv, output_RT,
                                                                      output_RTinv)
        plan = self.get_masks_for_batch(output_RT, input_RTinv, background_mask, compact=True)
        if self.vqvae is not None:
            target_codes = self.vqvae.encode_codes(output_img)
        elif "codes" in batch:
            target_codes = batch["codes"].to(dev)
        else:
            raise ValueError("forward_validation: no VQ-VAE: the batch must carry the target's codes")
        B, G = input_img.shape[0], self.obs[1]
        target_codes = target_codes.reshape(B, G, self.obs[2])
        score = self.autoreg_score(plan, target_codes)    # (a whole-grid pass alone: no column launch whose status would need reading)
        outputs = {"InputImg": input_img, "OutputImg": output_img, "PredDepthImg": regressed_pts / 5 - 1,
                   "ForegroundImg": (~background_mask).repeat(B, 1, 1, 1).float(), "FeaturesImg": gen_fs, "PredCodes": target_codes,
                   "NLLMap": score.nll.view(B, 1, G, self.obs[2]), "EntropyMap": score.entropy.view(B, 1, G, self.obs[2])}
        if self.vqvae is not None:
            outputs["PredImg"] = self._decode_checked(gen_fs, background_mask, target_codes.to(torch.int64))
        loss = {"autoreg_loss": score.mean_nll("all"), "ar_bits_per_code": score.bits_per_code("all"),
                "ar_bits_sampled": score.bits_per_code("sampled"), "ar_bits_observed": score.bits_per_code("observed"),
                "ar_accuracy_sampled": score.accuracy("sampled"), "ar_frames": score.frames}
        return loss, outputs

    # ---------------------------------------------------------------- sample ranking (8f.3, host logic)
    def _entropy_score(self, gen_img):
        """Entropy of the scene classifier on the candidate, including the reference's reinterpretation of the
        (3,256,256) tensor as (256,256,3) (z_buffermodel.py:256-262) and its 224x224 ImageNet-normalised input."""
        from PIL import Image
        raw = ((gen_img[0].reshape([256, 256, 3]).cpu().numpy() * .5 + .5) * 255).astype(np.uint8)
        im = np.asarray(Image.fromarray(raw).resize((224, 224), Image.BILINEAR), np.float32) / 255.0
        im = (im - np.array([0.485, 0.456, 0.406], np.float32)) / np.array([0.229, 0.224, 0.225], np.float32)
        x = torch.from_numpy(im).permute(2, 0, 1)[None].to(gen_img.device)
        with torch.no_grad():
            probs = torch.softmax(self.classifier(x).float().cpu(), 1).squeeze().numpy()
        probs = np.sort(probs)[::-1]
        return float(-np.sum(probs * np.log(probs)))

    def _decode_checked(self, gen_fs, background_mask, codes, check=True):
        """codes (B,32,32) -> image: decode, blend with the reprojected features (a14), refine -- one scope of the split-fp16 overflow guard
        (networks/f16x3.checked; check=False: unchecked).  Every image that is returned, ranked or fed into the next frame of a chain goes
        through here.  Weights under spectral norm behind normalisation layers do not overflow; a checkpoint that does should set
        opt.decoder_conv = "fp32" and save itself the first attempt."""
        return checked(gen_fs.device, lambda: self._project_checked(self.get_combined(gen_fs, self.vqvae.decode_code(codes), background_mask),
                                                                    background_mask), check)

    def _project_checked(self, x, *mask):
        """The refinement decoder, if the model has one, as a guarded scope; the no_outpainting form runs it on the reprojected features
        alone (z_buffermodel.py:383-384; the chained mode calls it without the mask argument)."""
        return x if self.projector is None else checked(x.device, lambda: self.projector(x, *mask))

    @torch.no_grad()
    def get_best_sample(self, *args, uniforms=None, shard=False, rank_on=None, rank_scope=None):
        """z_buffermodel.py:244-276 on the fused sampler: num_samples outpaintings of the same view, the best by
        discriminator + entropy rank is kept.  Two call forms:
          get_best_sample(gen_order, masks, downsampled_fs, background_mask, gen_fs, netD, input_img)   the reference's (:244),
              gen_order / masks as get_masks_for_batch returns them;
          get_best_sample(plan, codes, background_mask, gen_fs, netD, input_img)                         with the compact ARPlan.
        `codes` / downsampled_fs (B,32,32): the VQ-VAE codes of gen_fs.  One sample needs no scorers; more need `netD`
        (pixelsynth_amd.losses.DiscriminatorLoss or the reference's) and `self.classifier`.
        uniforms: optional (num_samples,B,L) draws (otherwise torch.Generator seeded i, as sample() reseeds with i).
        shard (or opt.shard_samples through forward_image): under torch.distributed the candidates are dealt over the ranks
        (candidate i on rank i % W: SURVEY 8e), two scalars per candidate are gathered, every rank applies the rank rule and
        the owner of the winner broadcasts it.
        rank_on "host": every candidate is scored as the reference scores it, one at a time through the host (run_discriminator_one_step,
        _entropy_score).  rank_on "device": the candidates, decoded exactly as on the host route, are stacked and scored in one batch
        where they are (ranking.score_candidates), the rank rule runs there too and the winner comes back through index_select -- no
        score comes down (under `shard`: the two vectors of a rank's own candidates, once).  It applies where ranking.can_score_on_device
        holds and B = 1; any other scorer, stand-ins included, takes the host route.  None: opt.rank_on, then the environment variable
        PS_RANK, "host" where neither is set.
        rank_scope "batch": the above -- with B > 1 views the host route averages the discriminator's score over the batch and takes the
        entropy of view 0, so the batch gets ONE winner index (the reference's rule).  rank_scope "view", with B > 1 and num_samples > 1:
        every view keeps the best of ITS candidates.  Candidate i of every view is drawn as a B = 1 run draws it (view_draws); the
        candidates are decoded as above, B views per call, stacked candidate-major to (num_samples * B,3,S,S), scored in chunks
        (ranking.score_candidates, opt.rank_chunk), ranked per view (ranking.select_groups) and every view's winner is handed over
        (ranking.take_groups) -> (B,3,S,S); no score and no index comes down.  This route exists on the device alone: it needs
        ranking.can_score_on_device and rank_on unset or "device" (NotImplementedError otherwise), and does not shard (ValueError).
        None: opt.rank_scope, then the environment variable PS_RANK_SCOPE, "batch" where neither is set."""
        from . import distributed as D
        from . import ranking
        route = _rank_route(rank_on, self.opt)
        scope = _rank_scope(rank_scope, self.opt)
        if isinstance(args[0], ARPlan):
            plan, codes, background_mask, gen_fs, netD, input_img = args
        else:
            gen_order, masks, codes, background_mask, gen_fs, netD, input_img = args
            plan = plan_from_reference_args(gen_order, masks, self.downsample(background_mask.float()), gen_fs.device)
        n = max(int(getattr(self.opt, "num_samples", 1)), 1)
        if n > 1 and (netD is None or self.classifier is None):
            raise RuntimeError("num_samples > 1 ranks candidates with the discriminator (netD: pixelsynth_amd.losses.DiscriminatorLoss "
                               "or the reference's) and the scene classifier -- pass netD or use num_samples=1")
        B, G = codes.shape[0], self.obs[1]
        L = G * self.obs[2]
        dev = codes.device
        per_view = scope == "view" and B > 1 and n > 1
        if per_view:
            if shard:
                raise ValueError("get_best_sample: rank_scope='view' does not shard its candidates over the ranks (shard=True)")
            asked = rank_on if rank_on is not None else getattr(self.opt, "rank_on", None) or os.environ.get("PS_RANK")
            if asked == "host" or not ranking.can_score_on_device(netD, self.classifier):
                raise NotImplementedError(f"get_best_sample: num_samples = {n} with rank_scope='view' and B = {B} ranks on the device alone: "
                                          "it needs scorers that ranking.can_score_on_device accepts and rank_on unset or 'device'")
            if uniforms is None:
                uniforms = view_draws(n, B, L).to(dev)
        if uniforms is None:
            uniforms = torch.stack([torch.rand(B, L, generator=torch.Generator(device="cpu").manual_seed(i)) for i in range(n)]).to(dev)
        rank, world = D.world()
        mine = D.shard_views(n, rank, world) if (shard and world > 1 and n > 1) else list(range(n))
        # The candidates are independent AR runs of the same view(s): they go through the sampler TOGETHER, as k * B frames
        # (sample-major) that share the view's order and masks and differ in their draws -- one wavefront schedule, the
        # launches of one run instead of k runs one after the other (the num_samples candidates are one of
        # the path's natural parallel axes).
        per = max(1, min(len(mine), self.sample_batch // max(B, 1)))          # candidates per engine run
        imgs, disc, entr, on_device = {}, [], [], None
        for s0 in range(0, len(mine), per):
            idx = mine[s0:s0 + per]
            k = len(idx)
            rep = lambda t: t.repeat((k,) + (1,) * (t.dim() - 1)).contiguous()
            waves = plan.waves
            if k > 1:
                waves = wavefronts(np.tile(plan.order_host, (k, 1)), G, self.obs[2], plan.first_step, dev)
            c = rep(codes.reshape(B, L).to(torch.int32))
            eng = self.outpaint2.engine(G, self.obs[2], k * B)
            eng.ar_run(c, rep(plan.order_loc), rep(plan.region), rep(plan.mask_init), rep(plan.mask_undilated),
                       rep(plan.mask_dilated), temperature=self.opt.temperature,
                       uniforms=uniforms[idx].reshape(k * B, L).contiguous(), first_step=plan.first_step, waves=waves)
            eng.check()
            for j, i in enumerate(idx):
                img = self._decode_checked(gen_fs, background_mask, c[j * B:(j + 1) * B].view(B, G, self.obs[2]))
                imgs[i] = img
                if per_view:
                    continue
                if n > 1 and on_device is None:
                    on_device = route == "device" and B == 1 and ranking.can_score_on_device(netD, self.classifier, img)
                if n > 1 and not on_device:
                    disc.append(float(netD.run_discriminator_one_step(img, input_img)["D_Fake"].mean().cpu()))
                    entr.append(self._entropy_score(img))
        if n == 1:
            return imgs[0]
        if per_view:
            stack = torch.cat([imgs[i] for i in range(n)])          # candidate-major: candidate i of view b at i * B + b
            if not ranking.can_score_on_device(netD, self.classifier, stack):
                raise NotImplementedError(f"get_best_sample: num_samples = {n} with rank_scope='view': ranking.can_score_on_device does "
                                          f"not take candidates of shape {tuple(stack.shape)} {stack.dtype}")
            chunk = getattr(self.opt, "rank_chunk", None) or ranking.SCORE_CHUNK      # (a cap on the scorers' memory)
            disc_dev, entr_dev = ranking.score_candidates(stack, netD, self.classifier, chunk)
            return ranking.take_groups(stack, ranking.select_groups(disc_dev, entr_dev, B, n), n)
        if on_device:
            stack = torch.cat([imgs[i] for i in mine])
            disc_dev, entr_dev = ranking.score_candidates(stack, netD, self.classifier)
            if len(mine) == n:
                return stack.index_select(0, ranking.select(disc_dev, entr_dev))
            disc, entr = torch.stack([disc_dev, entr_dev]).double().cpu().tolist()    # the one download of this rank's scores
        if len(mine) < n:
            d_all, e_all = D.gather_scores(disc, entr, n)
            best = rank_samples(list(d_all), list(e_all))
            return D.broadcast_from(imgs.get(best), D.owner_of(best, world), gen_fs.device)   # (a rank without candidates
                                                                                               # learns the shape from the owner)
        return imgs[rank_samples(disc, entr)]

    # ---------------------------------------------------------------- chained trajectories (8f.4)
    def _scene_depth(self, img, batch):
        if self.pts_regressor is not None:  # :476-480
            return torch.sigmoid(self.pts_regressor(img)) * (self.opt.max_z - self.opt.min_z) + self.opt.min_z
        fn = batch.get("depth_fn")  # synthetic runs: a callable img -> depth stands in for the Unet
        if fn is None:
            raise RuntimeError("forward_scene regresses depth from every generated frame: give the model a "
                               "pts_regressor or the batch a 'depth_fn' callable")
        return fn(img)

    def _scene_frame(self, st, batch, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv, netD, input_img):
        """One frame of a chained trajectory: depth of the current frame, cumulative reprojection (only the points
        that were background last time are new, a5), outpainting, state hand-over (:476-522 / :540-582)."""
        depth = self._scene_depth(st.img, batch)
        fs = st.img if getattr(self.opt, "use_rgb_features", True) else self.encoder(st.img)
        B = st.img.shape[0]
        cloud = feats = plan = uniforms = None
        if B == 1:
            gen_fs, background_mask, cloud, feats = self.pts_transformer.forward_justpts_cumulative(
                fs, depth, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv, st.cloud, st.feats, st.background, st.out_RTinv)
        else:
            gen_fs, background_mask = self._scene_step_batched(st, fs, depth, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv)
            # a scene is the same picture alone or in a batch: every scene gets the draws of a B = 1 run (candidate i: the (1, L)
            # draw of manual_seed(i)), never row b of a (B, L) draw
            uniforms = view_draws(max(int(getattr(self.opt, "num_samples", 1)), 1), B, self.obs[1] * self.obs[2]).to(gen_fs.device)
        if not getattr(self.opt, "no_outpainting", False):
            plan = build_ar_plan(background_mask, self.obs[1], count_background=B > 1)
            gen_img = self.get_best_sample(plan, self.vqvae.encode_codes(gen_fs), background_mask, gen_fs, netD, input_img,
                                           uniforms=uniforms, rank_scope="view" if B > 1 else None)   # (a batch of scenes ranks per scene)
        else:
            gen_img = self._project_checked(gen_fs)
        st.img, st.cloud, st.feats, st.background, st.out_RTinv = gen_img, cloud, feats, background_mask, out_RTinv
        st.new_counts = None if plan is None else plan.background_counts
        return gen_img, gen_fs, depth, background_mask

    SCENE_CAP_FRAMES = 2   # frames' worth of points (W * W each) a batched chain's state starts with; it doubles when a frame needs more

    def _scene_step_batched(self, st, fs, depth, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv):
        """The reprojection + splat of one frame of B > 1 chained scenes on their SceneState (PtsManipulator.forward_scene_step): the
        clouds stay on the device, every scene with its own length.  The host knows every scene's next count before the launch (the AR
        plan of the last frame counted its mask), so the state grows here, ahead of the step, and the step itself never overflows."""
        pm = self.pts_transformer
        B, C, W = fs.shape[0], fs.shape[1], pm.W
        if st.scenes is None:
            from .projection.z_buffer_manipulator import SceneState
            cap = int(getattr(self.opt, "scene_cap", 0) or self.SCENE_CAP_FRAMES * W * W)
            st.scenes = SceneState(B, C, max(cap, W * W), fs.device)
        new_counts = None
        if st.background is not None:
            new_counts = st.new_counts
            if new_counts is None:      # (no_outpainting: no plan has read the mask)
                new_counts = st.background.reshape(B, -1).sum(1, dtype=torch.int32).tolist()
            need = max(p + int(n) for p, n in zip(st.scenes.counts, new_counts))
            if need > st.scenes.cap:
                st.scenes = st.scenes.grown(max(need, 2 * st.scenes.cap))
        return pm.forward_scene_step(st.scenes, fs, depth, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv, st.background, st.out_RTinv,
                                     new_counts=new_counts)

    @torch.no_grad()
    def forward_scene(self, batch, netD=None):
        """z_buffermodel.py:420-584 (model_setting gen_scene / gen_two_imgs): per direction, first the far end of the
        sweep (unless sequential_outpainting), then the views in between, every frame rendered from the previous
        one on top of the accumulated point cloud.
        B = 1 runs as the reference does (a5 with boolean gathers, which need equal counts per image).  B > 1 -- images (B,3,S,S),
        cameras (B,4,4), for gen_two_imgs a (B,) "direction" -- advances B INDEPENDENT scenes one frame per step together, their
        clouds of different lengths kept on the device (_scene_step_batched); poses are built per scene and stacked, and slice b of
        every output equals the B = 1 run of scene b; with num_samples > 1 every scene keeps the best of its own candidates at every
        frame (get_best_sample's rank_scope="view": scorers that ranking.can_score_on_device accepts are needed).  With per-scene
        directions (gen_two_imgs) a value is stored under the key of every direction in the batch: slice b is scene b's under ITS
        direction's keys.
        -> (None, outputs) with the reference's keys PredImg_<dir>_<i>, FeaturesImg_..., PredDepthImg_..., ForegroundImg_...
        (ForegroundImg_* (B,1,S,S))."""
        dev = next(self.parameters()).device   # (the renderer itself refuses anything but the GPU)
        input_img = batch["images"][0].to(dev)
        cam = {k: v.to(dev) for k, v in batch["cameras"][0].items() if torch.is_tensor(v)}
        K, K_inv, input_RT, input_RTinv = cam["K"], cam["Kinv"], cam["P"], cam["Pinv"]
        two = self.opt.model_setting == 'gen_two_imgs'
        B = input_img.shape[0]
        if B == 1:
            directions = [self.mapping[int(batch["direction"])]] if two else list(self.opt.directions)
        else:
            if max(int(getattr(self.opt, "num_samples", 1)), 1) > 1:
                from . import ranking
                if netD is None or self.classifier is None or not ranking.can_score_on_device(netD, self.classifier):
                    raise NotImplementedError("forward_scene with B > 1 and num_samples > 1 ranks every scene's own candidates, which it "
                                              "does on the device alone: it needs netD and a classifier that ranking.can_score_on_device "
                                              "accepts -- or use num_samples = 1 or B = 1")
            if any(v.shape[0] != B for v in (K, K_inv, input_RT, input_RTinv)):
                raise ValueError(f"forward_scene: {B} images need (B,4,4) cameras")
            if two:   # one sweep, every scene in its own direction
                per_scene = [self.mapping[int(d)] for d in torch.as_tensor(batch["direction"]).reshape(-1).tolist()]
                if len(per_scene) != B:
                    raise ValueError(f"forward_scene: {B} images need a (B,) direction, got {len(per_scene)}")
                directions = [tuple(per_scene)]
            else:
                directions = list(self.opt.directions)
        sequential = bool(getattr(self.opt, "sequential_outpainting", False))
        outputs = {"InputImg": input_img}
        st = _SceneState(input_img)

        def pose_of(direction, numerator, denom):
            if B == 1:
                return self.get_rt_from_rot(direction, input_RT, numerator, denom)
            # per scene, as a B = 1 run builds them (a (1,4,4) inverse each), then stacked
            per = direction if isinstance(direction, tuple) else (direction,) * B
            pairs = [self.get_rt_from_rot(d, input_RT[b:b + 1], numerator, denom) for b, d in enumerate(per)]
            return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])

        def put(kind, direction, tag, value):
            for d in (dict.fromkeys(direction) if isinstance(direction, tuple) else (direction,)):
                outputs[f"{kind}_{d}_{tag}"] = value

        def summary(direction, tag, gen_fs, depth, background_mask):
            put("FeaturesImg", direction, tag, gen_fs)
            put("PredDepthImg", direction, tag, depth)
            # (B = 1: the reference's repeat(B, 1, 1, 1); its B x B result for a batch is not kept -- (B,1,S,S))
            put("ForegroundImg", direction, tag, ((~background_mask).repeat(B, 1, 1, 1) if B == 1 else (~background_mask).unsqueeze(1)).float())

        for direction in directions:
            base = int(self.opt.num_split)
            if two:
                num_split = 2
            elif direction in ('S', 'C'):
                num_split = base * 2
            elif direction in ('U', 'D', 'UL', 'UR', 'DR', 'DL'):
                num_split = max(base // 2, 1)
            else:
                num_split = base

            def source_pose():  # where the frame we render FROM was taken
                if st.numerator is None:
                    return input_RTinv, input_RT
                return pose_of(st.direction, st.numerator, num_split)

            if not sequential:
                # the large completion first (:470-522)
                in_RTinv, in_RT = source_pose()
                out_RTinv, out_RT = pose_of(direction, num_split, num_split)
                gen_img, gen_fs, depth, bgm = self._scene_frame(st, batch, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv,
                                                                netD, input_img)
                st.numerator, st.direction = num_split, direction
                put("PredImg", direction, num_split, gen_img)
                summary(direction, num_split, gen_fs, depth, bgm)
                todo = range(num_split - 1, -1, -1)
            else:
                todo = range(num_split + 1)
            for i in todo:
                if sequential and i == 0:
                    in_RTinv, in_RT = source_pose()
                else:
                    in_RTinv, in_RT = pose_of(direction, st.numerator, num_split)
                out_RTinv, out_RT = pose_of(direction, i, num_split)
                gen_img, gen_fs, depth, bgm = self._scene_frame(st, batch, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv,
                                                                netD, input_img)
                put("PredImg", direction, i, gen_img)
                put("FeaturesImg", direction, i, gen_fs)
                if sequential and i == num_split:
                    summary(direction, num_split, gen_fs, depth, bgm)
                    st.direction = direction
                st.numerator = i
        return None, outputs

    @torch.no_grad()
    def forward_gen_order(self, batch):
        """z_buffermodel.py:594-639 (model_setting 'get_gen_order'): depth, reprojection + splat, generation order --
        -> (None, {"gen_order": (B,L,2) int64 device tensor of (row, col) by rank})."""
        dev = next(self.parameters()).device
        input_img = batch["images"][0].to(dev)
        cam = {k: v.to(dev) for k, v in batch["cameras"][0].items() if torch.is_tensor(v)}
        K, K_inv, input_RT, input_RTinv = cam["K"], cam["Kinv"], cam["P"], cam["Pinv"]
        if len(batch["cameras"]) > 1 and "P" in batch["cameras"][-1]:   # process_batch hands over the target pose (:127-130) ...
            output_RT, output_RTinv = batch["cameras"][-1]["P"].to(dev), batch["cameras"][-1]["Pinv"].to(dev)
        else:                                                           # ... a demo-style batch has the direction instead
            output_RTinv, output_RT = self.get_rt_from_rot(self.opt.direction, input_RT)
        regressed_pts = self.regress_depth(input_img, batch["depths"][0].to(dev) if "depths" in batch else None)   # :606-612
        fs = input_img if getattr(self.opt, "use_rgb_features", True) else self.encoder(input_img)
        _, background_mask = self.pts_transformer.forward_justpts(fs, regressed_pts, K, K_inv, input_RT, input_RTinv,
                                                                  output_RT, output_RTinv)
        plan = self.get_masks_for_batch(output_RT, input_RTinv, background_mask, compact=True)
        return None, {"gen_order": torch.from_numpy(np.stack(plan.gen_order)).to(dev)}

    def forward(self, batch, netD=None):
        """z_buffermodel.py:278-290."""
        if self.opt.model_setting in ('gen_scene', 'gen_two_imgs'):
            return self.forward_scene(batch, netD)
        if self.opt.model_setting == 'get_gen_order':
            return self.forward_gen_order(batch)
        return self.forward_image(batch, netD)
