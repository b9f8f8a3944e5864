"""The batched AR run of ZbufferModelPts (z_buffermodel.py): V independent views planned (reproject + splat, generation order, masks)
and outpainted in one pass, and the pipeline that keeps the AR runs of consecutive batches in flight in one engine handle -- what bench.py
and driver.py live on.  OutpaintPipeline is a plain base class of the model: it has no state of its own and reads the model's
`pts_transformer`, `vqvae`, `obs` and `_engine`."""
import os

import numpy as np
import torch

from .ar_plan import build_ar_plan
from .lmconv.model import TP_MIN_FRAMES, LaunchPipeline, launch_capacity

_PREFIX_STREAMS = {}    # (device, n) -> the prefix pass's side streams (OutpaintPipeline._prefix_streams)


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


class OutpaintPipeline:
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
        eng = self._engine(V)
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
        eng = self._engine(st.sched.depth * V)
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
            self._pipe_step(self._engine(st.sched.depth * st.V), st, drain=True)
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
            self._engine(fs.shape[0]).check()
        return out
