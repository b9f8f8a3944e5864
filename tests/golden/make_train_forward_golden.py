"""Generate tests/golden/train_forward.npz by IMPORTING the reference (read-only) on the CPU, with make_golden.py's shims: the fixture
holds inputs and the reference's OUTPUTS only.  It never runs on a GPU machine.

(a) The reference's ZbufferModelPts.forward under model_setting 'train' (models/z_buffermodel.py:291-419) at B = 1, W = 256, ngf = 8,
    Unet 32, losses = ["1.0_l1"] (torchvision's VGG is not available here), in train() with the VQ-VAE in eval() (frozen: its codebook
    must not take an EMA step), for two cases: "depth_ar" (train_depth, lambda_autoreg = 1) and "pretrain".  Stand-ins, the same on
    this project's side of the comparison:
      * the renderer (pytorch3d) is replaced by one that returns a recorded (gen_fs, background_mask) pair: the oracle's projection +
        splat of the source image at a smooth depth, gen_fs rounded to fp16 (so that it can be stored as such, exactly);
      * get_masks_for_batch (cv2) is replaced by this project's masks (ps_ar_plan on the host) in the reference's layout;
      * forward_image's unbound `depth_img` (:316, :405) is bound to the source view's depth, batch["depths"][0];
      * the weights are this project's seeded model's (tests/_forward_train_util.py), loaded through load_state_dict.
    Recorded: gen_fs (fp16), the mask (bits), the decoder's noise and its seed, and per case every loss entry, the fp64 norm of every
    parameter's gradient after Total Loss.backward(), and the reference's own fp32-against-fp64 gap on each of them (the same module in
    double; for a gradient the fp64 norm of the difference of the two); PredImg once (it is the same in both cases: the splat is recorded), float32 on
    every second pixel.
(b) The reference's BaseModel.__call__ (models/base_model.py:81-148) twice in a row on a one-convolution stand-in generator at
    32 x 32 with ndf = 8, with and without normalize_image: the merged loss dicts, and every GRID-th value of every generator and
    discriminator parameter after each call.

Run:  python tests/golden/make_train_forward_golden.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the reference on the path; its shims are reused)
import _forward_train_util as U  # noqa: E402
from oracle import c_oracle as co  # noqa: E402
from pixelsynth_amd import _lib, synthetic as syn  # noqa: E402

NOISE_SEED, PRED_STEP, GRID = 5, 2, 7


def recorded_splat(batch, opt):
    """The oracle's projection + splat of the source image at a smooth depth -> (gen_fs (1,3,256,256) fp16-exact f32, bg (1,256,256) bool)"""
    src, dst = batch["cameras"]
    depth = syn.depth_smooth(U.SOURCE_SEED + 1, 1, 256, 1.0, 8.0)
    pts = co.project_pts(depth.reshape(1, 1, -1), src["K"].numpy(), src["Kinv"].numpy(), src["Pinv"].numpy(), dst["P"].numpy(), 256)
    feat = batch["images"][0].numpy().reshape(1, 3, -1)
    out = co.splat_forward(np.ascontiguousarray(pts.transpose(0, 2, 1)), feat, 256, radius_px=opt.radius, K=opt.pp_pixel, tau=opt.tau,
                           rad_pow=opt.rad_pow, accumulation=opt.accumulation, bg_ksize=opt.background_smoothing_kernel_size)
    return out["feat"].astype(np.float16).astype(np.float32), out["bg"]


def our_masks(bg):
    """This project's kernel masks of a (B,S,S) background mask, on the host (ps_ar_plan) -> three (B,9,L) f32 arrays"""
    B, S, _ = bg.shape
    L = 32 * 32
    order, region = np.empty((B, L), np.int32), np.empty((B, L), np.uint8)
    masks = [np.empty((B, 9, L), np.float32) for _ in range(3)]
    first = np.empty(1, np.int32)
    _lib.call("ps_ar_plan", np.ascontiguousarray(bg, dtype=np.uint8), B, S, 32, order, region, *masks, first)
    return masks, order


def reference_model(zb, kw, gen_fs, bg, dtype):
    """The reference's module with this project's seeded weights and the stand-ins of the docstring, in `dtype`"""
    opt = U.train_opts(**kw)
    ours = U.make_model(opt)
    real_available = torch.cuda.is_available
    torch.cuda.is_available = lambda: True          # SynthesisLoss keeps its terms only "on the device" (.cuda() is the identity here)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            model = zb.ZbufferModelPts(opt)
    finally:
        torch.cuda.is_available = real_available
    missing, unexpected = model.load_state_dict(ours.state_dict(), strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith(("encoder.", "classifier.")) or k in ("min_z", "max_z", "discretized_zs") for k in missing), missing
    model.train()
    model.vqvae.eval()
    for p in model.vqvae.parameters():
        p.requires_grad = False
    g, m = torch.from_numpy(gen_fs).to(dtype), torch.from_numpy(bg)
    model.pts_transformer.forward_justpts = lambda *a, **k: (g, m)
    masks, order = our_masks(bg)
    rep = lambda a, c: torch.from_numpy(a).unsqueeze(1).repeat(1, c, 1, 1).view(-1, 9, 1024).to(dtype)
    gen_order = [np.stack([o // 32, o % 32], 1).astype(np.int64) for o in order]
    model.get_masks_for_batch = lambda *a, **k: (rep(masks[0], 513), rep(masks[1], 160), rep(masks[2], 80), gen_order)
    return model


def reference_forward(zb, case, kw, batch, gen_fs, bg, fx):
    model = reference_model(zb, kw, gen_fs, bg, torch.float32)
    zb.depth_img = batch["depths"][0]               # (the name forward_image reads and never binds: a module global here)
    torch.manual_seed(NOISE_SEED)
    loss, out = model(batch)
    loss["Total Loss"].backward()
    keys = sorted(loss)
    fx[f"{case}_loss_keys"] = np.array(keys)
    fx[f"{case}_loss_values"] = np.array([float(loss[k].detach()) for k in keys], np.float64)
    assert set(out) == U.OUTPUT_KEYS, sorted(out)
    norms = U.grad_norms(model)
    grads32 = {k: p.grad.detach().double().clone() for k, p in model.named_parameters() if p.grad is not None}
    fx[f"{case}_grad_keys"] = np.array(sorted(norms))
    fx[f"{case}_grad_norms"] = np.array([norms[k] for k in sorted(norms)], np.float64)
    print(case, {k: round(float(loss[k].detach()), 6) for k in keys}, len(norms), "gradients")
    # The reference's OWN fp32-against-fp64 gap on every recorded quantity: the same module in double on the same inputs (the codes and
    # the decoded image are the fp32 run's: an argmin must not flip), the same noise draws widened.  A quantity that is cancellation
    # noise in fp32 -- the bias of a convolution in front of a batch norm has a gradient of exactly zero -- shows here as a gap of
    # its own size.
    with torch.no_grad():
        codes = model.vqvae.encode(batch["images"][-1])[3]
        decoded = model.vqvae.decode_code(codes).double()
    model = reference_model(zb, kw, gen_fs, bg, torch.float64).double()      # (a fresh module: a forward moves spectral-norm vectors and statistics)
    model.vqvae.encode = lambda x: (None, None, None, codes, None)
    model.vqvae.decode_code = lambda c: decoded
    real_randn = torch.randn
    wide = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    batch64 = dict(images=[wide(t) for t in batch["images"]], cameras=[{k: wide(v) for k, v in c.items()} for c in batch["cameras"]],
                   depths=[wide(t) for t in batch["depths"]])
    zb.depth_img = batch64["depths"][0]
    torch.randn = lambda *a, **k: real_randn(*a, **k).double()
    try:
        torch.manual_seed(NOISE_SEED)
        loss64, out64 = model(batch64)
        loss64["Total Loss"].backward()
    finally:
        torch.randn = real_randn
    grads64 = {k: p.grad.detach() for k, p in model.named_parameters() if p.grad is not None}
    fx[f"{case}_loss_gap"] = np.array([abs(float(loss64[k].detach()) - float(loss[k].detach())) for k in keys], np.float64)
    # (the norm of the DIFFERENCE, which bounds the difference of the norms: two vectors of cancellation noise agree in length by chance)
    fx[f"{case}_grad_gap"] = np.array([float((grads64[k] - grads32[k]).norm()) for k in sorted(norms)], np.float64)
    fx[f"{case}_pred_gap"] = np.array(float((out64["PredImg"].detach() - out["PredImg"].detach().double()).abs().max()))
    rel = fx[f"{case}_grad_gap"] / np.maximum(fx[f"{case}_grad_norms"], 1e-300)
    print(case, "fp32 against fp64: losses", fx[f"{case}_loss_gap"].max(), "PredImg", float(fx[f"{case}_pred_gap"]), "gradient norms: largest relative gap",
          rel.max(), "at", sorted(norms)[int(rel.argmax())], "; above 1e-3:", int((rel > 1e-3).sum()))
    return out["PredImg"].detach().numpy()


def step_record(trainer, batch, tag, fx):
    for call in range(2):
        losses, images = trainer(batch)
        keys = sorted(losses)
        fx[f"{tag}_call{call}_loss_keys"] = np.array(keys)
        fx[f"{tag}_call{call}_loss_values"] = np.array([float(losses[k].detach().mean()) for k in keys], np.float64)
        names = sorted(k for k, _ in trainer.named_parameters())
        params = dict(trainer.named_parameters())
        fx[f"{tag}_call{call}_param_keys"] = np.array(names)
        fx[f"{tag}_call{call}_params"] = np.concatenate([params[k].detach().reshape(-1)[::GRID].numpy() for k in names])
        fx[f"{tag}_call{call}_pred_range"] = np.array([float(images["PredImg"].min()), float(images["PredImg"].max())])
        print(tag, call, {k: round(float(losses[k].detach().mean()), 6) for k in keys})


def main():
    torch.set_num_threads(8)
    MG._import_reference()
    zb = MG._import_reference_model()
    fx = dict(noise_seed=np.array(NOISE_SEED), pred_step=np.array(PRED_STEP), grid=np.array(GRID))
    batch = U.make_batch(1)
    gen_fs, bg = recorded_splat(batch, U.train_opts())
    fx["gen_fs"], fx["bg_bits"] = gen_fs.astype(np.float16), np.packbits(bg.reshape(-1))
    print("recorded splat: background", float(bg.mean()))
    torch.manual_seed(NOISE_SEED)
    fx["noise"] = torch.stack([torch.randn(1, 20) for _ in range(16)]).numpy()
    preds = [reference_forward(zb, case, kw, batch, gen_fs, bg, fx)
             for case, kw in (("depth_ar", dict(train_depth=True, lambda_autoreg=1.0)), ("pretrain", dict(pretrain=True)))]
    assert np.array_equal(preds[0], preds[1]), "PredImg differs between the cases"
    fx["pred_img"] = preds[0][:, :, ::PRED_STEP, ::PRED_STEP].astype(np.float32)
    from models.base_model import BaseModel
    for tag, normalize in (("step_plain", False), ("step_normalized", True)):
        step_record(*U.step_setup(BaseModel, normalize), tag, fx)
    path = os.path.join(HERE, "train_forward.npz")
    np.savez_compressed(path, **fx)
    print("train_forward.npz", len(fx), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
