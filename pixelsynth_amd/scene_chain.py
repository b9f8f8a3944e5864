"""Chained trajectories of ZbufferModelPts (z_buffermodel.py): model_setting gen_scene / gen_two_imgs, every frame
rendered from the previous one on top of the accumulated point cloud, one scene or a batch of independent scenes.  SceneChain is a
plain base class of the model: it has no state of its own and reads the model's options, networks, `_source_view`, `_features`,
`num_samples`, `get_rt_from_rot` and `get_best_sample`."""
import torch

from . import ranking
from .ar_plan import build_ar_plan
from .best_sample import view_draws


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


def scene_num_split(base, direction, two):
    """Steps of the sweep in `direction` (z_buffermodel.py:455-468): opt.num_split, doubled for 'S' / 'C', halved for the vertical and
    diagonal directions; gen_two_imgs has two"""
    if two:
        return 2
    if direction in ('S', 'C'):
        return base * 2
    if direction in ('U', 'D', 'UL', 'UR', 'DR', 'DL'):
        return max(base // 2, 1)
    return base


def _put(outputs, kind, direction, tag, value):
    """outputs[<kind>_<direction>_<tag>]; with per-scene directions (a tuple) under the key of every direction in the batch"""
    for d in (dict.fromkeys(direction) if isinstance(direction, tuple) else (direction,)):
        outputs[f"{kind}_{d}_{tag}"] = value


class SceneChain:
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
        fs = self._features(st.img)
        B = st.img.shape[0]
        cloud = feats = plan = uniforms = None
        if B == 1:
            gen_fs, background_mask, cloud, feats = self.pts_transformer.forward_justpts_cumulative(
                fs, depth, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv, st.cloud, st.feats, st.background, st.out_RTinv)
        else:
            gen_fs, background_mask = self._scene_step_batched(st, fs, depth, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv)
            # a scene is the same picture alone or in a batch: every scene gets the draws of a B = 1 run (candidate i: the (1, L)
            # draw of manual_seed(i)), never row b of a (B, L) draw
            uniforms = view_draws(self.num_samples, B, self.obs[1] * self.obs[2]).to(gen_fs.device)
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

    def _scene_directions(self, batch, B):
        """The directions of the run, one sweep each: opt.directions, or for gen_two_imgs the one the batch carries -- B > 1: a (B,)
        "direction", one sweep with every scene in its own direction (a tuple)"""
        if self.opt.model_setting != 'gen_two_imgs':
            return list(self.opt.directions)
        if B == 1:
            return [self.mapping[int(batch["direction"])]]
        per_scene = [self.mapping[int(d)] for d in torch.as_tensor(batch["direction"]).reshape(-1).tolist()]
        if len(per_scene) != B:
            raise ValueError(f"forward_scene: {B} images need a (B,) direction, got {len(per_scene)}")
        return [tuple(per_scene)]

    def _scene_pose(self, B, direction, input_RT, numerator, denom):
        """get_rt_from_rot for the B scene(s) of input_RT (B,4,4); direction: one for all, or a tuple with one per scene"""
        if B == 1:
            return self.get_rt_from_rot(direction, input_RT, numerator, denom)
        # per scene, as a B = 1 run builds them (a (1,4,4) inverse each), then stacked
        per = direction if isinstance(direction, tuple) else (direction,) * B
        pairs = [self.get_rt_from_rot(d, input_RT[b:b + 1], numerator, denom) for b, d in enumerate(per)]
        return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])

    def _scene_sweep(self, st, batch, cams, direction, num_split, netD, outputs):
        """The frames of one direction (:470-584): the far end of the sweep first (the large completion, :470-522), then the views in
        between, back to the start -- or with sequential_outpainting from the start to the far end.  Every frame is rendered from where
        the run stands: the input, or the frame before -- for the first frame of a direction the last one of the direction before, its
        pose taken with THIS direction's num_split, as the reference takes it."""
        K, K_inv, input_RT, input_RTinv = cams
        pose_of = lambda d, numerator: self._scene_pose(st.img.shape[0], d, input_RT, numerator, num_split)
        sequential = bool(getattr(self.opt, "sequential_outpainting", False))
        for i in (range(num_split + 1) if sequential else range(num_split, -1, -1)):
            in_RTinv, in_RT = (input_RTinv, input_RT) if st.numerator is None else pose_of(st.direction, st.numerator)
            out_RTinv, out_RT = pose_of(direction, i)
            gen_img, gen_fs, depth, bgm = self._scene_frame(st, batch, K, K_inv, in_RT, in_RTinv, out_RT, out_RTinv, netD, outputs["InputImg"])
            _put(outputs, "PredImg", direction, i, gen_img)
            _put(outputs, "FeaturesImg", direction, i, gen_fs)
            if i == num_split:
                _put(outputs, "PredDepthImg", direction, i, depth)
                # ((B,1,S,S): at B = 1 the reference's repeat(B, 1, 1, 1); its B x B result for a batch is not kept)
                _put(outputs, "ForegroundImg", direction, i, (~bgm).unsqueeze(1).float())
            st.numerator, st.direction = i, direction

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
        _, input_img, *cams = self._source_view(batch)
        B = input_img.shape[0]
        if B > 1:
            if self.num_samples > 1:
                if netD is None or self.classifier is None or not ranking.can_score_on_device(netD, self.classifier):
                    raise NotImplementedError("forward_scene with B > 1 and num_samples > 1 ranks every scene's own candidates, which it "
                                              "does on the device alone: it needs netD and a classifier that ranking.can_score_on_device "
                                              "accepts -- or use num_samples = 1 or B = 1")
            if any(v.shape[0] != B for v in cams):
                raise ValueError(f"forward_scene: {B} images need (B,4,4) cameras")
        outputs = {"InputImg": input_img}
        st = _SceneState(input_img)
        for direction in self._scene_directions(batch, B):
            num_split = scene_num_split(int(self.opt.num_split), direction, self.opt.model_setting == 'gen_two_imgs')
            self._scene_sweep(st, batch, cams, direction, num_split, netD, outputs)
        return None, outputs
