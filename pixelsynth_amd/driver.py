"""Driver of the novel-view path (SURVEY 8b "what calls it"): the counterpart of the reference's demo.py:181-270 /
create_vid.py for what this repository builds.

    python -m pixelsynth_amd.driver --trajectory circle --frames 64 --out results/      (one GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
           -m pixelsynth_amd.driver --trajectory circle --frames 64 --out results/         (C4: views sharded over 8 GPUs)
    python -m pixelsynth_amd.driver --scene R L --num-split 4 --out results/             (chained, as the reference's gen_scene)
    python -m pixelsynth_amd.driver --scene R L --image-dir imgs/ --batch 16 --out results/   (many chained scenes, 16 at a time)
    python -m pixelsynth_amd.driver --pairs directions.npy --image-dir imgs/ --out views/  (gen_two_imgs: what evaluate --consistency scores)
    python -m pixelsynth_amd.driver --validate nll.json --image-dir src/ --target-dir tgt/ --trajectory R --out tf/   (teacher-forced)

One source image (a PNG, or the synthetic RealEstate10K-shaped sample), the demo cameras of process_demo_data
(demo.py:36-96), target poses from ZbufferModelPts.get_rt_from_rot (directions 'R','L','U','D',... in `--frames`
equal steps, or the 'C' circle of z_buffermodel.py:217-225).  Every view is rendered independently FROM THE SOURCE
(the reference's demo chains frames on one GPU): reproject + splat, VQ-VAE top codes, AR outpainting,
decode, get_combined.  Ranks take views round-robin, finished frames are all-gathered (RCCL), rank 0 writes
<out>/video/%d.png in trajectory order -- the layout create_vid.py's ffmpeg call expects (demo.py:125-164).

--scene runs ZbufferModelPts.forward_scene instead (z_buffermodel.py:420-584): frames chained on ONE GPU, each rendered
from the previous generated frame on top of the accumulated point cloud; images go to <out>/scene/ and <out>/video/ in
the reference's save_scene / save_video layout (demo.py:100-164).  A chain does not shard: with several ranks, rank r
renders its own chain for direction list r (replicas).

Several source images (--image A B ..., or --image-dir) are several INDEPENDENT scenes: with --scene they run through the batched
chained path in groups of --batch (forward_scene with B > 1: ragged clouds kept on the device) and are dealt over the ranks with
distributed.shard_views -- no collective, every rank writes its own scenes, scene i to <out>/<%04d>/scene/ and <out>/<%04d>/video/.
--pairs DIRECTIONS.npy (a 1-D array of direction indices into R L U D UL UR DR DL, one per image) runs gen_two_imgs the same way and
writes the layout of the reference's eval_consistency.py:122-149 under <out>/<%04d>/: input_image_.png,
output_image_<d>_0001.png, output_image_<d>_0002.png -- the views `python -m pixelsynth_amd.evaluate --consistency` lists.

--num-samples N with --discriminator PATH and --classifier PATH (state_dicts of losses.DiscriminatorLoss and of
networks.resnet18(num_classes=365)) is the reference's quality mode (num_samples 50 of its demo scripts) on the chained paths, --scene
and --pairs: every frame of every scene keeps the best of N outpaintings, scored and ranked on the device (pixelsynth_amd/ranking.py;
a batch of scenes ranks per scene).  The circle / trajectory path renders one sample per view.

--validate OUT.json scores held-out pairs instead of drawing anything (ZbufferModelPts.forward_validation, the reference's teacher-forced
forward, z_buffermodel.py:351-381): source i (--image / --image-dir) with target i, the images of --target-dir in sorted order; the source
has the demo cameras, the target's pose is the source's turned in the pair's direction at the model's rotation -- --trajectory DIR for
every pair, or per pair the index of --pairs DIRECTIONS.npy.  In batches of --batch: the target's VQ-VAE codes are scored under the
PixelCNN in the pair's generation order.  OUT.json gets the numbers of every pair (nats and bits per code, over all, the sampled and the
observed locations; the accuracy and mean entropy there) and their means over all the pairs' locations; with --out, the teacher-forced
predictions go to <out>/pred/<i>.png and the targets to <out>/gt/<i>.png, what `python -m pixelsynth_amd.evaluate --pred --gt` reads.
Nothing is downloaded: the checkpoints are --pixelcnn / --vqvae (random-init stand-ins without them, as everywhere here).

The depth regressor (networks.Unet) and the refinement decoder (networks.get_decoder) are part of the package, and ZbufferModelPts
builds them from the reference's options (norm_G, refine_model_type); THIS driver builds the model without them and ships no trained
weights: depth is synthetic unless --depth-npy is given, weights are random-init unless --pixelcnn / --vqvae state
dicts are given, and the saved image is the un-refined composite (reprojected features where visible, decoded sample elsewhere).
"""
import argparse
import os
import types

import numpy as np
import torch

from . import distributed as D, synthetic as syn
from .networks.f16x3 import checked


def make_opts(**kw):
    o = dict(W=256, use_rgb_features=True, splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=128,
             tau=1.0, rad_pow=2, accumulation="alphacomposite", background_smoothing_kernel_size=13, min_z=1.0, max_z=100.0,
             rotation=0.6, direction="R", temperature=0.7, model_setting="gen_scene", seed=0, homography=False, vqvae=True)
    o.update(kw)
    return types.SimpleNamespace(**o)


def build_scorers(discriminator_sd, classifier_sd):
    """--discriminator / --classifier -> (netD, classifier) of the sample ranking, on the host: the discriminator mirror in hinge mode
    (the options of the reference's trained model) and the Places365 ResNet-18, each with its state_dict loaded strictly."""
    from .losses import DiscriminatorLoss
    from .networks import resnet18
    opt = argparse.Namespace(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=64, output_nc=3,
                             no_ganFeat_loss=False, isTrain=False, lambda_feat=10.0)
    netD, classifier = DiscriminatorLoss(opt).eval(), resnet18(num_classes=365).eval()
    netD.load_state_dict(torch.load(discriminator_sd, map_location="cpu"), strict=True)
    classifier.load_state_dict(torch.load(classifier_sd, map_location="cpu"), strict=True)
    return netD, classifier


def build_model(device, pixelcnn_sd=None, vqvae_sd=None, classifier=None):
    from .z_buffermodel import ZbufferModelPts
    model = ZbufferModelPts(make_opts(), classifier=classifier).eval()
    load = lambda path, fallback: torch.load(path, map_location="cpu") if path else {k: torch.from_numpy(v) for k, v in fallback.items()}
    model.outpaint2.load_state_dict(load(pixelcnn_sd, syn.pixelcnn_state_dict(0)))
    model.vqvae.load_state_dict(load(vqvae_sd, syn.vqvae_state_dict(0)))
    return model.to(device)


def trajectory(model, input_RT, kind, n):
    """-> list of (label, RTinv (1,4,4), RT (1,4,4)) target poses, in playback order."""
    poses = []
    for i in range(n):
        if kind == "circle":
            inv, rt = model.get_rt_from_rot("C", input_RT, i, n)
            poses.append((f"C_{i}", inv, rt))
        else:
            inv, rt = model.get_rt_from_rot(kind, input_RT, i + 1, n)
            poses.append((f"{kind}_{i + 1}", inv, rt))
    return poses


@torch.no_grad()
def render_views(model, img, depth, cam, poses, temperature=0.7, seed=0):
    """img (1,3,S,S) in [-1,1], depth (1,1,S,S), cam dict of (1,4,4) tensors, poses as from trajectory()
    -> dict(frames (V,3,S,S), features, background_mask, codes): the views of `poses`, batched through outpaint_views.  One scope of the
    split-fp16 overflow guard (networks/f16x3.checked): checked once, rerun in fp32 if an activation left fp16's range."""
    V = len(poses)
    rep = lambda t: t.expand(V, *t.shape[1:]).contiguous()
    RT2 = torch.cat([p[2] for p in poses]).contiguous()
    RT2inv = torch.cat([p[1] for p in poses]).contiguous()
    g = torch.Generator(device="cpu").manual_seed(seed)
    uniforms = torch.rand(V, 1024, generator=g).to(img.device)

    def run():
        out = model.outpaint_views(rep(img), rep(depth), rep(cam["K"]), rep(cam["Kinv"]), rep(cam["P"]), rep(cam["Pinv"]), RT2, RT2inv,
                                   None, temperature=temperature, uniforms=uniforms)
        model.outpaint2.engine(32, 32, V).check()
        sample = model.vqvae.decode_code(out["codes"])
        frames = model.get_combined(out["gen_fs"], sample, out["background_mask"])
        return dict(frames=frames, features=out["gen_fs"], background_mask=out["background_mask"], codes=out["codes"])
    return checked(img.device, run)


def scene_outputs_to_disk(outputs, directions, num_split, out_dir):
    """PredImg_<dir>_<i> of forward_scene -> scene/output_image_<dir>_%04d.png (demo.py:100-123) and video/%d.png in
    playback order: out along each direction, and back again for the rotational ones (demo.py:125-164).
    -> number of video frames written."""
    def splits(d):
        return num_split * 2 if d in ("S", "C") else max(num_split // 2, 1) if d in ("U", "D", "UL", "UR", "DR", "DL") else num_split
    scene, vid = os.path.join(out_dir, "scene"), os.path.join(out_dir, "video")
    os.makedirs(scene, exist_ok=True)
    os.makedirs(vid, exist_ok=True)
    for d in directions:
        if d in ("S", "C"):
            continue
        for i in range(1, splits(d) + 1):
            save_png(os.path.join(scene, "output_image_%s_%04d.png" % (d, i)), outputs[f"PredImg_{d}_{i}"][0])
    save_png(os.path.join(vid, "0.png"), outputs[f"PredImg_{directions[0]}_0"][0])
    n = 1
    for d in directions:
        order = list(range(1, splits(d)))
        if d not in ("S", "C"):
            order += list(range(splits(d) - 1, -1, -1))
        for i in order:
            save_png(os.path.join(vid, f"{n}.png"), outputs[f"PredImg_{d}_{i}"][0])
            n += 1
    return n


MAPPING = ("R", "L", "U", "D", "UL", "UR", "DR", "DL")     # gen_two_imgs: index -> direction (eval_consistency.py:101)
IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg")


def source_images(image, image_dir):
    """--image / --image-dir -> the list of source paths, scene i = entry i (a directory's images in sorted order)."""
    paths = list(image or [])
    if image_dir:
        if paths:
            raise ValueError("--image and --image-dir exclude each other")
        paths = sorted(os.path.join(image_dir, f) for f in os.listdir(image_dir) if f.lower().endswith(IMAGE_SUFFIXES))
        if not paths:
            raise ValueError(f"--image-dir {image_dir}: no {' / '.join(IMAGE_SUFFIXES)} image")
    return paths


def load_directions(path, n_scenes):
    """--pairs DIRECTIONS.npy -> one direction index per scene (the file evaluate --consistency reads with --directions)."""
    dirs = np.load(path)
    if dirs.ndim != 1:
        raise ValueError(f"{path}: a 1-D array of direction indices expected, got shape {dirs.shape}")
    if len(dirs) < n_scenes:
        raise ValueError(f"{path} holds {len(dirs)} directions for {n_scenes} source images")
    dirs = [int(d) for d in dirs[:n_scenes]]
    for i, d in enumerate(dirs):
        if not 0 <= d < len(MAPPING):
            raise ValueError(f"{path}: item {i}: direction {d} outside 0 .. {len(MAPPING) - 1}")
    return dirs


def scene_groups(n_scenes, batch, rank, world):
    """The scenes of rank `rank`, dealt by distributed.shard_views, in groups of at most `batch` -> list of lists of scene indices.
    Over the ranks every scene appears exactly once."""
    if batch < 1:
        raise ValueError(f"--batch must be >= 1, got {batch}")
    mine = D.shard_views(n_scenes, rank, world)
    return [mine[s:s + batch] for s in range(0, len(mine), batch)]


def scene_dir(out_dir, index):
    return os.path.join(out_dir, "%04d" % index)


def scenes_to_disk(outputs, group, directions, num_split, out_dir):
    """The outputs of a batched forward_scene (gen_scene) -> scene_outputs_to_disk's layout inside <out>/<%04d>/ for every scene of
    `group` (slice b = scene group[b]).  -> video frames written per scene."""
    n = 0
    for b, index in enumerate(group):
        one = {k: v[b:b + 1] for k, v in outputs.items() if k.startswith("PredImg_")}
        n = scene_outputs_to_disk(one, directions, num_split, scene_dir(out_dir, index))
    return n


def pairs_to_disk(outputs, group, direction_ids, out_dir):
    """The outputs of a batched forward_scene (gen_two_imgs) -> eval_consistency.py:122-149 under <out>/<%04d>/ for every scene of
    `group`: the input and the views 1 and 2 of the scene's own direction."""
    for b, (index, d) in enumerate(zip(group, direction_ids)):
        name, folder = MAPPING[d], scene_dir(out_dir, index)
        os.makedirs(folder, exist_ok=True)
        save_png(os.path.join(folder, "input_image_.png"), outputs["InputImg"][b])
        for i in (1, 2):
            save_png(os.path.join(folder, "output_image_%s_%04d.png" % (name, i)), outputs[f"PredImg_{name}_{i}"][b])


@torch.no_grad()
def run_scenes(model, imgs, cam, groups, out_dir, directions=None, num_split=None, pair_directions=None, netD=None):
    """Independent chained scenes in batches: imgs {scene index: (1,3,S,S)}, cam the (1,4,4) demo cameras every scene starts from,
    groups from scene_groups.  pair_directions {scene index: direction index}: gen_two_imgs and the --pairs layout; otherwise
    gen_scene over `directions` and the per-scene scene/ + video/ layout.  netD: the discriminator of the sample ranking
    (opt.num_samples > 1).  -> scenes written."""
    done = 0
    for group in groups:
        B = len(group)
        batch = {"images": [torch.cat([imgs[i] for i in group])], "depth_fn": syn.depth_from_image,
                 "cameras": [{k: v.expand(B, 4, 4).contiguous() for k, v in cam.items()}]}
        if pair_directions is not None:
            ids = [pair_directions[i] for i in group]
            batch["direction"] = torch.tensor(ids)
        _, outputs = model(batch, netD)
        model.outpaint2.engine(32, 32, B).check()
        if pair_directions is not None:
            pairs_to_disk(outputs, group, ids, out_dir)
        else:
            scenes_to_disk(outputs, group, directions, num_split, out_dir)
        done += B
    return done


def validation_setup(args, error):
    """--validate: the arguments checked before any device is touched -> (source paths, target paths, direction index per pair).
    error: the parser's (raises SystemExit)."""
    if args.scene:
        error("--validate and --scene exclude each other")
    if args.num_samples != 1:
        error("--validate draws no sample: --num-samples does not apply")
    if int(os.environ.get("WORLD_SIZE", 1)) > 1:
        error("--validate runs on one GPU")
    if args.batch < 1:
        error(f"--batch must be >= 1, got {args.batch}")
    if not args.target_dir:
        error("--validate needs --target-dir DIR, the target image of every source")
    try:
        sources = source_images(args.image, args.image_dir)
        targets = source_images(None, args.target_dir) if sources else []
    except (ValueError, OSError) as err:
        error(str(err).replace("--image-dir " + str(args.target_dir), "--target-dir " + str(args.target_dir)))
    if not sources:
        error("--validate needs --image ... or --image-dir, the source images")
    if len(targets) != len(sources):
        error(f"--validate: {len(sources)} source images and {len(targets)} images in --target-dir {args.target_dir}: pair i is source i "
              "and target i, in sorted order")
    if args.pairs:
        try:
            ids = load_directions(args.pairs, len(sources))
        except (ValueError, OSError) as err:
            error(str(err))
    elif args.trajectory in MAPPING:
        ids = [MAPPING.index(args.trajectory)] * len(sources)
    else:
        error(f"--validate: the target's pose is the source's turned in a direction: --trajectory {' | '.join(MAPPING)} (got "
              f"{args.trajectory!r}) or --pairs DIRECTIONS.npy")
    return sources, targets, ids


def validation_numbers(frames):
    """A (N,2,4) frames table of likelihood.CodeNLL (any device) -> per row forward_validation's numbers, the mean entropies and the group sizes, as lists of
    N floats (NaN: a group without a location)"""
    from .likelihood import CodeNLL
    s = CodeNLL(None, None, None, frames.detach().double().cpu())
    cols = {"autoreg_loss": s.mean_nll("all", True), "ar_bits_per_code": s.bits_per_code("all", True),
            "ar_bits_sampled": s.bits_per_code("sampled", True), "ar_bits_observed": s.bits_per_code("observed", True),
            "ar_accuracy_sampled": s.accuracy("sampled", True), "ar_entropy_bits_sampled": s.mean_entropy_bits("sampled", True),
            "ar_entropy_bits_observed": s.mean_entropy_bits("observed", True),
            "n_sampled": s.sums("sampled", True)[:, 0], "n_observed": s.sums("observed", True)[:, 0]}
    return {k: v.tolist() for k, v in cols.items()}


def validation_report(frames, sources, targets, direction_ids):
    """The (N,2,4) frames table of N pairs -> what --validate writes: {"pairs": [per pair its files, direction and numbers], "mean":
    the same numbers over ALL the pairs' locations of a group (for autoreg_loss, 1024 locations a pair, the mean of the pairs'),
    "count": N}; NaN is written as null"""
    clean = lambda v: None if v != v else v
    per = validation_numbers(frames)
    pooled = validation_numbers(frames.sum(0, keepdim=True))
    pairs = [dict(index=i, source=sources[i], target=targets[i], direction=MAPPING[direction_ids[i]],
                  **{k: clean(v[i]) for k, v in per.items()}) for i in range(len(sources))]
    return {"count": len(pairs), "temperature": 1.0, "mean": {k: clean(v[0]) for k, v in pooled.items()}, "pairs": pairs}


@torch.no_grad()
def run_validation(model, sources, targets, direction_ids, cam, batch, out_dir=None):
    """forward_validation over the pairs in batches of `batch`: cam the (1,4,4) demo cameras of every source; pair i's target pose is
    get_rt_from_rot(direction i) of it.  out_dir: PredImg to <out_dir>/pred/<i>.png, the target to <out_dir>/gt/<i>.png.
    -> the (N,2,4) frames table of the pairs, on the device."""
    device = cam["P"].device
    poses = {d: model.get_rt_from_rot(MAPPING[d], cam["P"]) for d in sorted(set(direction_ids))}     # (RTinv, RT)
    if out_dir:
        for sub in ("pred", "gt"):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    tables = []
    for s0 in range(0, len(sources), batch):
        idx = list(range(s0, min(s0 + batch, len(sources))))
        B = len(idx)
        src = torch.cat([load_image(sources[i]) for i in idx]).to(device)
        tgt = torch.cat([load_image(targets[i]) for i in idx]).to(device)
        cam0 = {k: v.expand(B, 4, 4).contiguous() for k, v in cam.items()}
        cam1 = dict(cam0, P=torch.cat([poses[direction_ids[i]][1] for i in idx]), Pinv=torch.cat([poses[direction_ids[i]][0] for i in idx]))
        loss, outputs = model.forward_validation({"images": [src, tgt], "cameras": [cam0, cam1], "depths": [syn.depth_from_image(src)]})
        tables.append(loss["ar_frames"])
        if out_dir:
            for b, i in enumerate(idx):
                save_png(os.path.join(out_dir, "pred", f"{i}.png"), outputs["PredImg"][b])
                save_png(os.path.join(out_dir, "gt", f"{i}.png"), outputs["OutputImg"][b])
    return torch.cat(tables)


_SIDE = {}


def _side_stream():
    """ONE side stream per device and process.  The runtime deals the streams a process creates onto a few hardware queues in turn,
    and one of every eight shares the main stream's queue -- its kernels then run behind the main stream's instead of beside them
    (docs/LAB_NOTEBOOK.md, "Which stream the side stream is": +25 % per step).  A stream created once, early, is the same stream on every call."""
    dev = torch.cuda.current_device()
    if dev not in _SIDE:
        _SIDE[dev] = torch.cuda.Stream()
    return _SIDE[dev]


@torch.no_grad()
def render_pipelined(model, img, depth, cam, chunks, seeds, temperature=0.7):
    """render_views for several batches of poses (seeds: per batch, one seed per view), with the host half of batch i + 1 (splat on a side stream, masks back,
    orders / masks / wavefront schedule, uploads) overlapped with the AR run of batch i.  -> list of frames (V_i,3,S,S).  One scope of the
    overflow guard, as render_views (on an exception the pipeline is reset: outpaint_reset)."""
    def run():
        main, side = torch.cuda.current_stream(), _side_stream()

        def inputs(chunk):
            V = len(chunk)
            rep = lambda t: t.expand(V, *t.shape[1:]).contiguous()
            return (rep(img), rep(depth), rep(cam["K"]), rep(cam["Kinv"]), rep(cam["P"]), rep(cam["Pinv"]),
                    torch.cat([p[2] for p in chunk]).contiguous(), torch.cat([p[1] for p in chunk]).contiguous())

        frames, planned = [], None
        # batches of one size (a trajectory cut into equal chunks): their AR runs overlap -- the narrow last wavefronts of a batch inside the
        # launches of the next batch's first ones (outpaint_pipelined; the same codes); a batch then comes back one call late
        overlap = len(chunks) > 1 and len({len(c) for c in chunks}) == 1 and len(chunks[0]) >= 2

        def finish(out):
            if out is not None:
                sample = model.vqvae.decode_code(out["codes"])
                frames.append(model.get_combined(out["gen_fs"], sample, out["background_mask"]))
        try:
            for k, chunk in enumerate(chunks):
                if planned is None:
                    planned = model.plan_views(*inputs(chunk))
                V = len(chunk)
                # the draws of a view are seeded by the VIEW (its index in the trajectory), not by where the sharding put it: a frame is
                # the same picture on one GPU or eight
                uniforms = torch.stack([torch.rand(1024, generator=torch.Generator(device="cpu").manual_seed(int(sd))) for sd in seeds[k]]).to(img.device)
                out = (model.outpaint_pipelined if overlap else model.outpaint_planned)(planned, None, temperature=temperature, uniforms=uniforms)
                planned = None
                if k + 1 < len(chunks):
                    if k == 0:
                        side.wait_stream(main)      # (the shared inputs were produced on the main stream)
                    with torch.cuda.stream(side):
                        planned = model.plan_views(*inputs(chunks[k + 1]))
                    model.adopt_planned(planned, main)
                    main.wait_stream(side)
                finish(out)
            if overlap:
                for out in model.outpaint_flush():
                    finish(out)
        except BaseException:
            model.outpaint_reset()      # (a batch left in flight must not be merged into the next sequence's launches)
            raise
        if chunks:
            model.outpaint2.engine(32, 32, len(chunks[-1])).check()
        return frames
    return checked(img.device, run)


def save_png(path, chw):
    """chw: (3,S,S) uint8 image, or float in [-1, 1]."""
    from PIL import Image
    if chw.dtype != torch.uint8:
        chw = D.to_image_u8(chw)
    Image.fromarray(chw.permute(1, 2, 0).cpu().numpy()).save(path)


def load_image(path, S=256):
    from PIL import Image
    im = Image.open(path).convert("RGB").resize((S, S), Image.BICUBIC)
    return torch.from_numpy(np.asarray(im).astype(np.float32) / 127.5 - 1.0).permute(2, 0, 1)[None]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--image", nargs="+", metavar="PATH", help="source PNG/JPEG (default: the synthetic sample); several: one scene each "
                                                                 "(with --scene or --pairs)")
    ap.add_argument("--image-dir", help="a directory of source images, one scene each, in sorted order (with --scene or --pairs)")
    ap.add_argument("--pairs", metavar="DIRECTIONS.npy", help="gen_two_imgs: per image the direction index of this 1-D array; writes "
                                                             "<out>/<%%04d>/{input_image_,output_image_<d>_0001,output_image_<d>_0002}.png")
    ap.add_argument("--depth-npy", help="(S,S) float32 depth in [min_z, max_z] (default: synthetic smooth depth)")
    ap.add_argument("--trajectory", default="circle", help="circle | R | L | U | D | UL | UR | DL | DR")
    ap.add_argument("--scene", nargs="+", metavar="DIR", help="chained mode: directions of forward_scene, e.g. R L C")
    ap.add_argument("--num-split", type=int, default=4, help="--scene: views per direction (num_split)")
    ap.add_argument("--sequential", action="store_true", help="--scene: sequential_outpainting")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16, help="views (or, with several images, chained scenes) rendered together per rank")
    ap.add_argument("--out", default=None, help="output directory (default: results; with --validate: no images unless given)")
    ap.add_argument("--validate", metavar="OUT.json", help="teacher-forced validation of (source, target) pairs: the likelihood of every "
                                                          "target's codes under the PixelCNN, as JSON")
    ap.add_argument("--target-dir", help="--validate: a directory of target images, target i (sorted order) for source i")
    ap.add_argument("--pixelcnn", help="state_dict of the reference's OurPixelCNN (torch.save)")
    ap.add_argument("--vqvae", help="state_dict of the reference's VQVAETop (torch.save)")
    ap.add_argument("--num-samples", type=int, default=1, metavar="N", help="--scene / --pairs: outpaintings per frame, the best by "
                                                                            "discriminator + entropy rank is kept (needs both scorers)")
    ap.add_argument("--discriminator", metavar="PATH", help="state_dict of losses.DiscriminatorLoss (torch.save)")
    ap.add_argument("--classifier", metavar="PATH", help="state_dict of networks.resnet18(num_classes=365), the Places365 classifier")
    args = ap.parse_args(argv)
    if args.num_samples < 1:
        ap.error("--num-samples must be >= 1")
    if args.num_samples > 1 and not (args.discriminator and args.classifier):
        ap.error("--num-samples > 1 ranks candidates with two scorers: give --discriminator PATH and --classifier PATH")
    if args.target_dir and not args.validate:
        ap.error("--target-dir goes with --validate OUT.json")
    if args.validate:
        sources, targets, ids = validation_setup(args, ap.error)
        return validate_main(args, sources, targets, ids)
    if args.out is None:
        args.out = "results"
    sources = source_images(args.image, args.image_dir)
    many = args.image_dir is not None or len(sources) > 1 or args.pairs is not None
    if many and not (args.scene or args.pairs):
        ap.error("several source images are several chained scenes: give --scene DIR ... or --pairs DIRECTIONS.npy")
    if args.scene and args.pairs:
        ap.error("--scene and --pairs exclude each other")
    if args.pairs and not sources:
        ap.error("--pairs needs --image ... or --image-dir")
    pair_ids = load_directions(args.pairs, len(sources)) if args.pairs else None

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    # PS_DRYRUN_ONE_GPU=1: every rank uses cuda:0 and the gloo backend -- the multi-rank control flow (sharding, gather, who
    # writes what) on a single-GPU box
    dry = os.environ.get("PS_DRYRUN_ONE_GPU") == "1"
    if dry:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if dry:
            torch.distributed.init_process_group("gloo")
        else:
            torch.distributed.init_process_group("nccl", device_id=device)
    netD = classifier = None
    ranked = args.num_samples > 1 and bool(args.scene or args.pairs)       # (the circle / trajectory path stays at one sample)
    if ranked:
        netD, classifier = build_scorers(args.discriminator, args.classifier)
        netD = netD.to(device)
    model = build_model(device, args.pixelcnn, args.vqvae, classifier)
    model.opt.num_samples = args.num_samples if ranked else 1
    if ranked:
        model.opt.rank_on = "device"     # (a trailing group of one scene scores on the same route as the groups before it)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if many:     # independent scenes: dealt over the ranks, no collective, every rank writes its own
        groups = scene_groups(len(sources), args.batch, rank, world)
        imgs = {i: load_image(sources[i]).to(device) for g in groups for i in g}
        cam = {k: t(v) for k, v in syn.demo_cameras(1).items()}
        if args.pairs:
            model.opt.model_setting, model.opt.num_split = "gen_two_imgs", 2      # (gen_two_imgs renders views 2, 1, 0 whatever num_split says)
            n = run_scenes(model, imgs, cam, groups, args.out, pair_directions=dict(enumerate(pair_ids)), netD=netD)
        else:
            model.opt.directions, model.opt.num_split, model.opt.sequential_outpainting = list(args.scene), args.num_split, args.sequential
            n = run_scenes(model, imgs, cam, groups, args.out, directions=list(args.scene), num_split=args.num_split, netD=netD)
        print(f"rank {rank}: {n} of {len(sources)} scenes ({'pairs' if args.pairs else 'chained ' + ' '.join(args.scene)}) in groups of "
              f"{args.batch} -> {args.out}/%04d/")
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    img = (load_image(sources[0]) if sources else torch.from_numpy(syn.image(1000, 1, 3, 256))).to(device)
    depth = t(np.load(args.depth_npy)[None, None].astype(np.float32)) if args.depth_npy else t(syn.depth_smooth(2000, 1, 256, 1.0, 100.0))
    cam = {k: t(v) for k, v in syn.demo_cameras(1).items()}
    if args.scene:
        model.opt.directions, model.opt.num_split = list(args.scene), args.num_split
        model.opt.sequential_outpainting = args.sequential
        batch = {"images": [img], "cameras": [cam], "depth_fn": syn.depth_from_image}
        _, outputs = model(batch, netD)
        model.outpaint2.engine(32, 32, 1).check()
        n = scene_outputs_to_disk(outputs, model.opt.directions, args.num_split, os.path.join(args.out, f"rank{rank}") if world > 1 else args.out)
        print(f"rank {rank}: chained scene {' '.join(args.scene)}: {n} video frames")
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    kind = "circle" if args.trajectory == "circle" else args.trajectory
    poses = trajectory(model, cam["P"], kind, args.frames)
    mine = D.shard_views(len(poses), rank, world)
    frames = render_pipelined(model, img, depth, cam, [[poses[i] for i in mine[s:s + args.batch]] for s in range(0, len(mine), args.batch)],
                              seeds=[[1000 + i for i in mine[s:s + args.batch]] for s in range(0, len(mine), args.batch)])
    local_frames = D.to_image_u8(torch.cat(frames)) if frames else torch.empty(0, 3, 256, 256, dtype=torch.uint8, device=device)
    per_rank = (len(poses) + world - 1) // world                         # gather_frames wants equal shards: pad the last round
    if local_frames.shape[0] < per_rank:
        pad = torch.zeros(per_rank - local_frames.shape[0], 3, 256, 256, dtype=torch.uint8, device=device)
        local_frames = torch.cat([local_frames, pad])
    all_frames = D.gather_frames(local_frames, len(poses))
    if rank == 0:
        vid = os.path.join(args.out, "video")
        os.makedirs(vid, exist_ok=True)
        save_png(os.path.join(vid, "0.png"), img[0])                      # frame 0 = the source (demo.py:133-137)
        for i in range(len(poses)):
            save_png(os.path.join(vid, f"{i + 1}.png"), all_frames[i])
        print(f"wrote {len(poses) + 1} frames to {vid}/%d.png  (ffmpeg -i {vid}/%d.png ... as create_vid.py does)")
    if world > 1:
        torch.distributed.destroy_process_group()


def validate_main(args, sources, targets, ids):
    """--validate: one GPU, forward_validation over the pairs, OUT.json (and the images under --out)"""
    import json
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_model(device, args.pixelcnn, args.vqvae)
    model.opt.model_setting = "gen_paired_img"       # (get_rt_from_rot: the direction at opt.rotation, not a step of a sweep)
    cam = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in syn.demo_cameras(1).items()}
    frames = run_validation(model, sources, targets, ids, cam, args.batch, args.out)
    report = validation_report(frames, sources, targets, ids)
    folder = os.path.dirname(os.path.abspath(args.validate))
    os.makedirs(folder, exist_ok=True)
    with open(args.validate, "w") as fh:
        json.dump(report, fh, indent=1)
    m = report["mean"]
    print(f"{report['count']} pairs: autoreg_loss {m['autoreg_loss']:.4f} nats, {m['ar_bits_per_code']:.4f} bits per code -> {args.validate}"
          + (f"; teacher-forced predictions -> {args.out}/pred, targets -> {args.out}/gt" if args.out else ""))


if __name__ == "__main__":
    main()
