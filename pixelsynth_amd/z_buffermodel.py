"""View-synthesis orchestration of the hot path -- counterpart of the reference's
models/z_buffermodel.py:ZbufferModelPts for the rows of SURVEY.md 8(a): target poses
(get_rt_from_rot :202-242), reprojection + splat (forward_justpts), generation order + masks
(get_masks_for_batch :641-701), autoregressive outpainting (get_best_sample -> sample()) and the
foreground/background blend (get_combined :703-708).

This file holds the reference-shaped model: the constructor, the poses, the depth rule, the entry points forward() dispatches to and
get_best_sample.  The class draws its other parts from plain base classes -- the batched AR run and its pipeline from
outpaint.OutpaintPipeline, the chained trajectories (forward_scene) from scene_chain.SceneChain -- and best-of-N is the free
functions of best_sample.py; their names are importable from here as before.

The dense networks the reference runs around that path are SURVEY 8(f) "next" rows: the VQ-VAE-2 top level
(pixelsynth_amd/vqvae2), the depth Unet and the refinement decoder (pixelsynth_amd/networks) are built when the
options name them (`vqvae`, `norm_G` + `refine_model_type`) or can be injected (`pts_regressor`, `vqvae`,
`projector`); the discriminator / Places365 classifier of the sample ranking are injected only.  When a network is
absent the batch must carry the tensors it would have produced (`depths`, `codes`) -- that is how the synthetic
benchmark drives the hot path on its own.
"""
import math
import types

import numpy as np
import torch
import torch.nn as nn

from . import best_sample, distributed as D, ranking
from .ar_plan import ARPlan, build_ar_plan, plan_from_reference_args
from .best_sample import RANK_ROUTES, RANK_SCOPES, _rank_route, _rank_scope, rank_samples, view_draws  # noqa: F401 (re-exported)
from .lmconv.layers import PONO
from .lmconv.model import OurPixelCNN
from .lmconv.sample import sample
from .networks import train_glue
from .networks.f16x3 import checked
from .outpaint import OutpaintPipeline
from .projection.z_buffer_manipulator import PtsManipulator
from .scene_chain import SceneChain


class ZbufferModelPts(OutpaintPipeline, SceneChain, nn.Module):
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
        if classifier is None and self.num_samples > 1:   # z_buffermodel.py:88 (random init until the
            from .networks import resnet18                  # Places365 state_dict is loaded, demo.py:233-243)
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
        if getattr(opt, "losses", None):   # z_buffermodel.py:94 (the training options carry the list; an inference model has no loss)
            from .losses.synthesis import SynthesisLoss
            self.loss_function = SynthesisLoss(opt)

    # ---------------------------------------------------------------- what every entry point reads off the options and the batch
    @property
    def num_samples(self):
        """opt.num_samples, 1 at least: the candidates get_best_sample ranks"""
        return max(int(getattr(self.opt, "num_samples", 1)), 1)

    def _engine(self, frames):
        """The PixelCNN engine handle of `frames` code grids"""
        return self.outpaint2.engine(self.obs[1], self.obs[2], frames)

    def _features(self, img):
        """What is splatted: the image itself, or the encoder's features of it"""
        return img if getattr(self.opt, "use_rgb_features", True) else self.encoder(img)

    def _source_view(self, batch):
        """The source view of a batch, on the model's device -> (device, image, K, Kinv, P, Pinv)"""
        dev = next(self.parameters()).device   # (the renderer itself refuses anything but the GPU)
        cam = {k: v.to(dev) for k, v in batch["cameras"][0].items() if torch.is_tensor(v)}
        return dev, batch["images"][0].to(dev), cam["K"], cam["Kinv"], cam["P"], cam["Pinv"]

    def _reproject(self, batch, carried):
        """What forward_image, forward_validation and forward_gen_order begin with: the source view, the target pose -- the one the
        batch carries (`carried`; process_batch :127-130) or the one of opt.direction --, the depth of the source image (:303-311 /
        :606-612), its features, reprojection + splat into the target pose.
        -> (device, input_img, regressed_pts, gen_fs, background_mask, and what get_masks_for_batch takes first: output_RT, input_RTinv)"""
        dev, input_img, K, K_inv, input_RT, input_RTinv = self._source_view(batch)
        if carried:
            output_RT, output_RTinv = batch["cameras"][-1]["P"].to(dev), batch["cameras"][-1]["Pinv"].to(dev)
        else:
            output_RTinv, output_RT = self.get_rt_from_rot(self.opt.direction, input_RT)
        regressed_pts = self.regress_depth(input_img, batch["depths"][0].to(dev) if "depths" in batch else None)
        gen_fs, background_mask = self.pts_transformer.forward_justpts(self._features(input_img), regressed_pts, K, K_inv, input_RT,
                                                                      input_RTinv, output_RT, output_RTinv)
        return dev, input_img, regressed_pts, gen_fs, background_mask, output_RT, input_RTinv

    @staticmethod
    def _view_outputs(input_img, regressed_pts, gen_fs, background_mask):
        """The output keys every reprojected view has"""
        return {"InputImg": input_img, "PredDepthImg": regressed_pts / 5 - 1,
                "ForegroundImg": (~background_mask).repeat(input_img.shape[0], 1, 1, 1).float(), "FeaturesImg": gen_fs}

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

    # ---------------------------------------------------------------- the batched hot path (outpaint.py), end to end
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
        fs_src = self._features(src_imgs)
        planned = self.plan_views(fs_src[view_src].contiguous(), depth_src[view_src].contiguous(), K, K_inv, input_RT, input_RTinv,
                                  output_RT, output_RTinv)
        out = self.outpaint_planned(planned, None, self.opt.temperature if temperature is None else temperature, uniforms)
        if check:
            self._engine(K.shape[0]).check()
        pred = self._decode_checked(out["gen_fs"], out["background_mask"], out["codes"], check)
        return dict(PredImg=pred, FeaturesImg=out["gen_fs"], background_mask=out["background_mask"], codes=out["codes"],
                    depth=depth_src, plan=out["plan"])

    # ---------------------------------------------------------------- reference-shaped single image path
    @torch.no_grad()
    def forward_image(self, batch, netD=None, rank_on=None):
        """Hot-path part of forward_image (z_buffermodel.py:291-419) for model_setting gen_img / gen_paired_img.
        batch: {"images": [(B,3,S,S)], "cameras": [{"P","Pinv","K","Kinv"}], optional "depths": [(B,1,S,S)],
        optional "codes": (B,32,32)} -> (None, outputs dict with the reference's keys).  rank_on: get_best_sample's."""
        paired = getattr(self.opt, "model_setting", "gen_img") == "gen_paired_img"   # :294-295: the target view comes with the batch
        dev, input_img, regressed_pts, gen_fs, background_mask, output_RT, input_RTinv = self._reproject(batch, paired)
        outputs = self._view_outputs(input_img, regressed_pts, gen_fs, background_mask)
        if paired:
            outputs["OutputImg"] = batch["images"][-1].to(dev)
        if getattr(self.opt, "no_outpainting", False):   # :383-384
            outputs["PredImg"] = self._project_checked(gen_fs, None)
            return None, outputs
        if self.vqvae is not None:
            enc = getattr(self.vqvae, "encode_codes", None)      # our mirror: top codes only, int32, on the device
            downsampled_fs = enc(gen_fs) if enc is not None else self.vqvae.encode(gen_fs)[3]
        else:
            downsampled_fs = batch["codes"].to(dev)
        if self.num_samples > 1:   # :349 -> get_best_sample with opt.num_samples candidates
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
        dev, input_img, regressed_pts, gen_fs, background_mask, output_RT, input_RTinv = self._reproject(batch, True)
        output_img = batch["images"][-1].to(dev)
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
        outputs = dict(self._view_outputs(input_img, regressed_pts, gen_fs, background_mask), OutputImg=output_img, PredCodes=target_codes,
                       NLLMap=score.nll.view(B, 1, G, self.obs[2]), EntropyMap=score.entropy.view(B, 1, G, self.obs[2]))
        if self.vqvae is not None:
            outputs["PredImg"] = self._decode_checked(gen_fs, background_mask, target_codes.to(torch.int64))
        loss = {"autoreg_loss": score.mean_nll("all"), "ar_bits_per_code": score.bits_per_code("all"),
                "ar_bits_sampled": score.bits_per_code("sampled"), "ar_bits_observed": score.bits_per_code("observed"),
                "ar_accuracy_sampled": score.accuracy("sampled"), "ar_frames": score.frames}
        return loss, outputs

    # ---------------------------------------------------------------- the generator's training forward (z_buffermodel.py:291-419, 'train')
    def forward_train(self, batch):
        """The reference's forward_image with model_setting 'train' (z_buffermodel.py:291-419) as a DIFFERENTIABLE method, what
        BaseModel (base_model.py) takes a step on.  batch: images [source, ..., target], cameras [source, ..., target], optional
        "depths" (the source view's, (B,1,S,S)) for opt.use_gt_depth / opt.train_depth.  -> (loss, outputs) as the reference.
          depth      the regressor's output through networks.train_glue.depth_head (:303-314), in grad mode; the given depth with
                     opt.use_gt_depth (or where the model has no regressor)
          splat      _features, then pts_transformer.forward_justpts: differentiable in the depth and the features (csrc/splat_bwd.hip)
          opt.no_outpainting   PredImg = projector(gen_fs, None), no AR term (:383-384)
          otherwise  the compact plan from the background mask, codes = vqvae.encode_codes(target) and input_gt =
                     vqvae.decode_code(codes), all three without gradients (the VQ-VAE is frozen: train_dpr.py:431-433); unless
                     opt.pretrain, autoreg_loss = likelihood.ar_loss over ALL locations at T = 1 (what nn.CrossEntropyLoss() gives at
                     :362); the decoder's input is train_glue.combine_mask_nhwc(gen_fs, input_gt, background_mask) -- blend, mask
                     channel and channels-last copy in one pass --, or, with opt.predict_residual (which adds the 3-channel blend to
                     the decoder's output), get_combined and the decoder's own concatenation
          loss       loss_function(PredImg, target) (SynthesisLoss, built where opt.losses exists); "autoreg_loss" = autoreg_loss /
                     (B * prod(obs) * ln 2) * 1000 -- obs = [3,32,32], so the reference's stray factor 3 is kept --, "Total Loss" +=
                     autoreg_loss * opt.lambda_autoreg (or += autoreg_loss where that option is absent or None); with opt.train_depth
                     "depth_loss" = L1(depth, batch["depths"][0]) is added and reported.  The reference reads a `depth_img` there that
                     its forward_image never binds (:316, :405); the SOURCE view's depth is this project's reading of it.
                     Both additions are IN PLACE, as the reference writes them (:400-406): where opt.losses names a single term,
                     SynthesisLoss hands that term's tensor out under both names, so the reported "L1" is then the total as well --
                     the reference's logs show the same number, and the fixture recorded from it holds this to it.
          outputs    InputImg, PredImg, PredDepthImg, ForegroundImg, OutputImg; no FeaturesImg (:385-417)
        A model without a VQ-VAE would take the reference's mixture-of-logistics branch (:364-368, :374): NotImplementedError."""
        opt = self.opt
        if len(batch["images"]) < 2 or len(batch["cameras"]) < 2:
            raise ValueError("forward_train: the batch carries the target view, images [source, target] and cameras [source, target]")
        if not hasattr(self, "loss_function"):
            raise RuntimeError("forward_train: the model has no loss_function (opt.losses names the terms of SynthesisLoss)")
        dev, input_img, K, K_inv, input_RT, input_RTinv = self._source_view(batch)
        output_img = batch["images"][-1].to(dev)
        output_RT, output_RTinv = batch["cameras"][-1]["P"].to(dev), batch["cameras"][-1]["Pinv"].to(dev)
        given = batch["depths"][0].to(dev) if "depths" in batch else None
        if self.pts_regressor is None or getattr(opt, "use_gt_depth", False):
            if given is None:
                raise ValueError("no depth regressor (or opt.use_gt_depth): the batch must carry the depth")
            regressed_pts, pred_depth = given, given / 5 - 1
        else:
            inverse = bool(getattr(opt, "use_inverse_depth", False))
            regressed_pts, pred_depth = train_glue.depth_head(self.pts_regressor(input_img), int(inverse), getattr(opt, "min_z", 0.0),
                                                              getattr(opt, "max_z", 0.0), opt)
        gen_fs, background_mask = self.pts_transformer.forward_justpts(self._features(input_img), regressed_pts, K, K_inv, input_RT,
                                                                      input_RTinv, output_RT, output_RTinv)
        autoreg_loss = None
        if getattr(opt, "no_outpainting", False):
            gen_img = gen_fs if self.projector is None else self.projector(gen_fs, None)
        else:
            if self.vqvae is None:
                raise NotImplementedError("forward_train: a model without a VQ-VAE trains the PixelCNN with the reference's "
                                          "mixture-of-logistics loss (discretized_mix_logistic_loss, z_buffermodel.py:364-368), which is "
                                          "not built")
            with torch.no_grad():
                codes = self.vqvae.encode_codes(output_img)
                input_gt = self.vqvae.decode_code(codes.to(torch.int64))
            if not getattr(opt, "pretrain", False):
                from .likelihood import ar_loss
                with torch.no_grad():
                    plan = self.get_masks_for_batch(output_RT, input_RTinv, background_mask, compact=True)
                autoreg_loss = ar_loss(self, codes.reshape(-1, self.obs[1], self.obs[2]), plan, group="all")
            if self.projector is None:
                gen_img = self.get_combined(gen_fs, input_gt, background_mask)
            elif getattr(opt, "predict_residual", False):
                gen_img = self.projector(self.get_combined(gen_fs, input_gt, background_mask), background_mask)
            else:
                gen_img = self.projector(train_glue.combine_mask_nhwc(gen_fs, input_gt, background_mask, opt))
        outputs = {"InputImg": input_img, "PredImg": gen_img, "PredDepthImg": pred_depth,
                   "ForegroundImg": (~background_mask).repeat(input_img.shape[0], 1, 1, 1).float()}
        loss = self.loss_function(gen_img, output_img)
        if autoreg_loss is not None:
            loss["autoreg_loss"] = autoreg_loss / (input_img.shape[0] * np.prod(self.obs) * np.log(2.)) * 1000
            lam = getattr(opt, "lambda_autoreg", None)
            loss["Total Loss"] += autoreg_loss if lam is None else autoreg_loss * lam      # (in place, as the reference: see the docstring)
        if getattr(opt, "train_depth", False):
            if given is None:
                raise ValueError("forward_train: opt.train_depth needs the source view's depth, batch['depths'][0]")
            depth_loss = nn.L1Loss()(regressed_pts, given)
            loss["Total Loss"] += depth_loss
            loss["depth_loss"] = depth_loss
        outputs["OutputImg"] = output_img
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
        route = _rank_route(rank_on, self.opt)
        scope = _rank_scope(rank_scope, self.opt)
        if isinstance(args[0], ARPlan):
            plan, codes, background_mask, gen_fs, netD, input_img = args
        else:
            gen_order, masks, codes, background_mask, gen_fs, netD, input_img = args
            plan = plan_from_reference_args(gen_order, masks, self.downsample(background_mask.float()), gen_fs.device)
        n = self.num_samples
        if n > 1 and (netD is None or self.classifier is None):
            raise RuntimeError("num_samples > 1 ranks candidates with the discriminator (netD: pixelsynth_amd.losses.DiscriminatorLoss "
                               "or the reference's) and the scene classifier -- pass netD or use num_samples=1")
        B, L = codes.shape[0], self.obs[1] * self.obs[2]
        per_view = scope == "view" and B > 1 and n > 1
        if per_view:
            if shard:
                raise ValueError("get_best_sample: rank_scope='view' does not shard its candidates over the ranks (shard=True)")
            asked = best_sample.resolve_option(rank_on, self.opt, "rank_on", "PS_RANK", RANK_ROUTES, None)
            if asked == "host" or not ranking.can_score_on_device(netD, self.classifier):
                raise NotImplementedError(f"get_best_sample: num_samples = {n} with rank_scope='view' and B = {B} ranks on the device alone: "
                                          "it needs scorers that ranking.can_score_on_device accepts and rank_on unset or 'device'")
        if uniforms is None:
            uniforms = view_draws(n, B, L) if per_view else torch.stack(
                [torch.rand(B, L, generator=torch.Generator(device="cpu").manual_seed(i)) for i in range(n)])
            uniforms = uniforms.to(codes.device)
        rank, world = D.world()
        mine = D.shard_views(n, rank, world) if (shard and world > 1 and n > 1) else list(range(n))
        cands = best_sample.candidates(self, plan, codes, background_mask, gen_fs, uniforms, mine)
        if n == 1:
            return next(cands)[1]
        if per_view:
            return best_sample.rank_per_view(self, cands, netD, n, B)
        first, cands = best_sample.peek(cands)      # the route is decided from the first decoded candidate
        if first is not None and route == "device" and B == 1 and ranking.can_score_on_device(netD, self.classifier, first):
            return best_sample.rank_on_device(self, cands, netD, n, world, gen_fs.device)
        return best_sample.rank_on_host(self, cands, netD, input_img, n, world, gen_fs.device)

    @torch.no_grad()
    def forward_gen_order(self, batch):
        """z_buffermodel.py:594-639 (model_setting 'get_gen_order'): depth, reprojection + splat, generation order --
        -> (None, {"gen_order": (B,L,2) int64 device tensor of (row, col) by rank})."""
        # process_batch hands over the target pose (:127-130); a demo-style batch has the direction instead
        carried = len(batch["cameras"]) > 1 and "P" in batch["cameras"][-1]
        dev, _, _, _, background_mask, output_RT, input_RTinv = self._reproject(batch, carried)
        plan = self.get_masks_for_batch(output_RT, input_RTinv, background_mask, compact=True)
        return None, {"gen_order": torch.from_numpy(np.stack(plan.gen_order)).to(dev)}

    def forward(self, batch, netD=None):
        """z_buffermodel.py:278-290."""
        if self.opt.model_setting in ('gen_scene', 'gen_two_imgs'):
            return self.forward_scene(batch, netD)
        if self.opt.model_setting == 'get_gen_order':
            return self.forward_gen_order(batch)
        if self.opt.model_setting == 'train':
            return self.forward_train(batch)
        return self.forward_image(batch, netD)
