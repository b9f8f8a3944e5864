"""Measurement: one optimiser step of the whole generator as the reference's train_dpr.py takes it -- base_model.BaseModel on
ZbufferModelPts.forward_train -- and what it costs by part.

    python tools/train_step_time.py [--pairs 4 16] [--ngf 64] [--ndf 64] [--unet 32] [--rounds 5] [--calls 3] [--profile-calls 2]

Workload: B pairs of 256 x 256 (B = 4 and 16), Unet 32, ngf 64, ndf 64, losses ["1.0_l1", "10.0_content"] with a rand-init VGG19, the
PixelCNN as the model builds it, the discriminator on, predict_residual off (so that the decoder's input is the fused blend; the
reference's scripts set it, and forward_train then takes the torch blend: docstring there).  A call is one BaseModel step: forward, the
generator's backward and Adam step, the discriminator's forward, backward and Adam step.

Five routes alternate call by call between device events (_measure.alternate) on the same model and batch: "hip", the step under
training.hip_routes() (every opt-in training kernel on), "default", every switch where the process has it, "hip+disc", the step
under training.hip_routes_with_discriminator() (the discriminator's 4 x 4 convolutions through csrc/disc_conv.hip as well), and "hip+sn",
the step under training.hip_routes_with_spectral() (the spectral normalisation of the decoder's, the Unet's and the discriminator's layers
as one batched pass per forward, csrc/spectral_train.hip).  A fifth, "hip+sn+unet", is the step under training.hip_routes_with_unet():
the depth Unet's norms, skip joins and wide 3 x 3 convolutions on HIP as well (networks/unet_train.py; its kernels stay in the class
"Unet", by the range around the regressor's forward).  After the warm-up calls
a round is CALLS calls per route and gives one median per route; the range of the ROUNDS medians is reported, with
torch.cuda.max_memory_allocated of each route (the largest over its calls, reset before every call).  The yardstick for either number is the other, of the
same tree in the same process; nothing else is claimed.

Then each route once more under torch's profiler, in a run of its own (_measure's protocol: CPU and device activities, PROFILE_CALLS
calls): device time by CLASS (_measure.by_range).  A kernel belongs to the class of the part of the step that launched it -- the parts are
marked with torch.profiler.record_function ranges around the modules' forwards and the optimisers' steps, a backward kernel goes to the class
of the forward operation it differentiates (the profiler's sequence numbers) -- refined by the kernel's name where a part holds several
classes (the PixelCNN: masked convolutions against the rest; the decoder: convolutions, norms, joins) and for the new glue kernels
and the k_sn_* kernels of the batched spectral norm ("spectral norm"), which are found by name wherever they run.  What no rule reaches is "everything else"; its largest names are listed.  One JSON line
per batch size."""
import argparse
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pixelsynth_amd import synthetic as syn, training  # noqa: E402
from pixelsynth_amd.base_model import BaseModel  # noqa: E402
from pixelsynth_amd.z_buffermodel import ZbufferModelPts  # noqa: E402
from _measure import alternate, by_range, marked as _marked, span  # noqa: E402

CLASSES = ("Unet", "splat forward", "splat backward", "planning", "VQ-VAE", "masked convolutions", "PixelCNN kernels",
           "decoder convolutions", "decoder norms", "decoder joins", "content loss", "discriminator convolutions", "discriminator rest",
           "glue kernels", "spectral norm", "optimisers", "everything else")
GLUE = ("k_combine_fwd", "k_combine_bwd", "k_depth_fwd", "k_depth_bwd")
SPECTRAL = ("k_sn_wtu", "k_sn_wv", "k_sn_v", "k_sn_u", "k_sn_div", "k_sn_dot", "k_sn_dw")      # csrc/spectral_train.hip
CONV_NAMES = ("conv", "Conv", "gemm", "Gemm", "GEMM", "Cijk", "igemm", "Igemm", "miopen", "MIOpen", "naive_", "gridwise", "col2im", "im2col",
              "Im2Col", "Col2Im", "wrw", "bwd_data", "xdlops", "SubTensorOp", "batched_transpose", "transpose_", "k_thin", "k_f16x3", "k_wgrad")
LMCONV_NAMES = ("k_gemm", "k_nchw_to_cl", "k_to_cl", "k_pack_conv", "k_reduce_nchw", "k_adjoint_mask", "k_grad_weight", "k_grad_bias")   # csrc/lmconv*.hip
NORM_NAMES = ("norm", "Norm", "k_stats", "k_apply", "welford", "Welford")
PREFIX = "ps_step::"
ROUTES = {"hip": training.hip_routes, "default": contextlib.nullcontext, "hip+disc": training.hip_routes_with_discriminator}
SPECTRAL_ROUTES = {"hip+sn": training.hip_routes_with_spectral}        # measured beside ROUTES
UNET_ROUTES = {"hip+sn+unet": training.hip_routes_with_unet}           # and beside those


def refine(part, kernel):
    """The class of a device event `kernel` launched inside the marked part `part` (None: outside every range)"""
    if any(k in kernel for k in GLUE):
        return "glue kernels"
    if any(k in kernel for k in SPECTRAL):
        return "spectral norm"
    if part == "pixelcnn":
        return "masked convolutions" if any(s in kernel for s in LMCONV_NAMES) else "PixelCNN kernels"
    if part == "decoder":
        return "decoder convolutions" if any(s in kernel for s in CONV_NAMES) else "decoder norms" if any(s in kernel for s in NORM_NAMES) else "decoder joins"
    if part == "discriminator":
        return "discriminator convolutions" if any(s in kernel for s in CONV_NAMES) else "discriminator rest"
    if part == "splat":
        return "splat forward"
    if part == "splat backward":
        return "splat backward"
    return {"unet": "Unet", "planning": "planning", "vqvae": "VQ-VAE", "content loss": "content loss", "optimisers": "optimisers"}.get(part, "everything else")


def marked(fn, part):
    return _marked(fn, PREFIX + part)


def mark_parts(trainer):
    """record_function ranges around the parts of a step (instance attributes: the classes stay as they are)"""
    m = trainer.model
    m.pts_regressor.forward = marked(m.pts_regressor.forward, "unet")
    m.pts_transformer.forward_justpts = marked(m.pts_transformer.forward_justpts, "splat")
    m.get_masks_for_batch = marked(m.get_masks_for_batch, "planning")
    m.vqvae.encode_codes = marked(m.vqvae.encode_codes, "vqvae")
    m.vqvae.decode_code = marked(m.vqvae.decode_code, "vqvae")
    m.outpaint2._forward_layers = marked(m.outpaint2._forward_layers, "pixelcnn")
    m.projector.forward = marked(m.projector.forward, "decoder")
    for term in m.loss_function.losses:        # the VGG19 term alone: L1, PSNR and SSIM stay in "everything else"
        if type(term).__name__ == "PerceptualLoss":
            term.forward = marked(term.forward, "content loss")
    trainer.netD.netD.forward = marked(trainer.netD.netD.forward, "discriminator")
    for opt in (trainer.optimizer_G, trainer.optimizer_D):
        opt.step = marked(opt.step, "optimisers")


def by_class(fn, calls):
    """-> ({class: device ms per call}, [(kernel name, ms per call)] the largest of "everything else")"""
    totals, rest = {c: 0.0 for c in CLASSES}, {}
    for part, backward, kernel, ms in by_range(fn, calls, PREFIX):
        cls = refine("splat backward" if part == "splat" and backward else part, kernel)
        totals[cls] += ms
        if cls == "everything else":
            rest[kernel[:70]] = rest.get(kernel[:70], 0.0) + ms
    top = sorted(rest.items(), key=lambda kv: -kv[1])[:8]
    return {c: round(v / calls, 3) for c, v in totals.items()}, [(n, round(v / calls, 3)) for n, v in top]


def train_opts(args):
    return argparse.Namespace(
        norm_G="sync:spectral_batch", refine_model_type="resnet_256W8UpDown3", ngf=args.ngf, predict_residual=False, normalize_before_residual=False,
        W=256, use_rgb_features=True, depth_predictor_type="unet", Unet_num_filters=args.unet, seed=0, min_z=0.5, max_z=10.0, voxel_size=64,
        model_setting="train", rotation=0.6, direction="R", homography=False, temperature=0.7, losses=["1.0_l1", "10.0_content"], vgg19_rand=True,
        discriminator_losses="pix2pixHD", splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=128, tau=1.0, rad_pow=2,
        accumulation="alphacomposite", background_smoothing_kernel_size=13, vqvae=True, use_gt_depth=False, use_inverse_depth=False,
        train_depth=False, isTrain=True, lr=1e-3, lr_d=2e-3, lr_g=5e-4, beta1=0.0, beta2=0.9, init="", normalize_image=True, num_samples=1,
        gan_mode="hinge", norm_D="spectralinstance", ndf=args.ndf, output_nc=3, no_ganFeat_loss=False, lambda_feat=10.0, niter=100, niter_decay=10)


def make_batch(B, device):
    t = lambda a: torch.from_numpy(a).to(device)
    cam = syn.demo_cameras(B)
    RTinv, RT = syn.yaw_pose(cam["P"], 0.35)
    src = {k: t(cam[k]) for k in ("K", "Kinv", "P", "Pinv")}
    return dict(images=[t(syn.image(301, B, 3, 256)), t(syn.image(302, B, 3, 256))], cameras=[src, dict(src, P=t(RT), Pinv=t(RTinv))])


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--ndf", type=int, default=64)
    ap.add_argument("--unet", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--profile-calls", type=int, default=2)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    opt = train_opts(args)
    torch.manual_seed(0)
    model = ZbufferModelPts(opt).train()
    for p in model.vqvae.parameters():
        p.requires_grad = False
    trainer = BaseModel(model, opt).to(device)
    mark_parts(trainer)
    routes = dict(ROUTES, **SPECTRAL_ROUTES, **UNET_ROUTES)
    for B in args.pairs:
        batch = make_batch(B, device)
        peak = {}

        def step(route):
            torch.cuda.reset_peak_memory_stats()      # (every call's peak is its own route's)
            with routes[route]():
                trainer(batch)
            peak[route] = max(peak.get(route, 0), torch.cuda.max_memory_allocated())
        med = alternate({route: (lambda r=route: step(r)) for route in routes}, args.rounds, args.calls, warm=2)
        classes = {}
        for route in routes:
            totals, rest = by_class(lambda: step(route), args.profile_calls)
            classes[route] = dict(device_ms_per_call=totals, everything_else_top=rest, device_ms_total=round(sum(totals.values()), 3))
        rec = dict(what="train_step", pairs=B, ngf=args.ngf, ndf=args.ndf, unet=args.unet, rounds=args.rounds, calls=args.calls,
                   hip_ms_median_range=span(med["hip"]), default_ms_median_range=span(med["default"]),
                   hip_disc_ms_median_range=span(med["hip+disc"]), hip_sn_ms_median_range=span(med["hip+sn"]),
                   hip_sn_unet_ms_median_range=span(med["hip+sn+unet"]),
                   max_memory_allocated_mb={k: round(v / 2 ** 20, 1) for k, v in peak.items()}, classes=classes)
        print("%d pairs: hip routes %.1f .. %.1f ms, default routes %.1f .. %.1f ms, hip routes with the discriminator's convolutions %.1f .. %.1f ms, "
              "hip routes with the batched spectral norm %.1f .. %.1f ms, with the Unet's route on top %.1f .. %.1f ms (medians of %d rounds of %d "
              "steps); peak memory %s MB"
              % (B, *span(med["hip"]), *span(med["default"]), *span(med["hip+disc"]), *span(med["hip+sn"]), *span(med["hip+sn+unet"]), args.rounds, args.calls,
                 rec["max_memory_allocated_mb"]))
        for c in CLASSES:
            print("  %-28s " % c + "   ".join("%s %9.3f ms" % (r, classes[r]["device_ms_per_call"][c]) for r in routes))
        print(json.dumps(rec), flush=True)
        del batch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
