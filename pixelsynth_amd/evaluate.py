"""Score predicted views against ground truth: PSNR and SSIM on the HIP kernel (csrc/metrics.hip) and, with --vgg16, PercSim (the
VGG16 perceptual similarity, perceptual.py) and, with --inception, FID (the Fréchet distance of Inception-v3 features, fid.py,
csrc/fid.hip); the reference's calc_errors_quality.py.

    python -m pixelsynth_amd.evaluate --pred DIR --gt DIR [--sampled DIR] [--max-img N] [--batch 64] [--json PATH] [--vgg16 PATH]
                                      [--inception PATH]

Image i is <dir>/<i>.png in each directory.  Without --max-img, i runs from 0 as long as --pred has <i>.png; with it, every i < N must be
there.  Images are read as RGB.  With --sampled, a pixel is "vis" where all channels of the ground truth equal the sampled image
(calc_errors_quality.py:28-35), which adds PSNR_vis / PSNR_invis and SSIM_vis / SSIM_invis.  One line per metric, its mean over the
images (PSNR clamped at 100 first, as the reference does).  --json writes the per-image rows and the means.  --vgg16 names VGG16
weights (torchvision's vgg16-397923af.pth, or a PNet state dict; nothing is downloaded) and adds PercSim -- with --sampled also
PercSim_invis and PercSim_vis, the images times the mask -- after the SSIM lines, means of the per-image values (no clamp).
--inception names Inception-v3 weights (pytorch_fid's pt_inception-2015-12-05-*.pth, or any state dict with torchvision's Inception3
keys; nothing is downloaded) and adds the line FID after the means: the Fréchet distance between the 2048-feature statistics of the
--pred images and of the --gt images (what `python -m pytorch_fid PRED GT` scores), the images the other metrics read, decoded once.
Under torch.distributed.run the feature rows travel with the metric rows and rank 0 does the statistics.

PNGs are decoded on a host thread pool (at most 16 threads), uploaded as pinned uint8 batches and scored on uint8 (the kernel converts
x / 255, TF.to_tensor's values); the next batch decodes while the device scores this one, one synchronisation per batch.  Under
torch.distributed.run the images are dealt with distributed.shard_views and the rows come back to every rank through one all-gather
(distributed.gather_rows); rank 0 prints and writes.  PS_DRYRUN_ONE_GPU=1 runs every rank on cuda:0 over gloo.

    python -m pixelsynth_amd.evaluate --consistency DIR --masks DIR --points DIR --directions FILE.npy [--vgg16 PATH] [--max-img N]
                                      [--batch B] [--json PATH]

scores the homography consistency of view pairs as calc_errors_consistency_homography.py does (consistency.py, csrc/consistency.hip):
item i (i < len(directions), or < N) has DIR/%04d/output_image_<d>_0001.png and _0002.png, d = consistency.MAPPING[directions[i]],
--masks DIR/%04d/mask1.png and mask2.png, --points DIR/reproj1_<i>.npy and reproj2_<i>.npy, frames of 256 x 256.  Prints PSNR_vis
-- with --vgg16 PercSim_vis first -- the mean over items of 0.5 (dir0 + dir1), PSNR clamped at 100 per direction.  The same decode
pool, pinned uploads and sharding as above.
"""
import argparse
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import distributed as D
from .image_metrics import COLUMNS, image_metrics
from . import consistency as CS
from .perceptual import COLUMNS as PERCSIM_COLUMNS, perceptual_rows
from . import fid as FID

PSNR_CLAMP = 100.0
# printed name -> column; the reference's names (calc_errors_quality.py:47-67) and their SSIM counterparts
NAMES = {"PSNR": "psnr", "PSNR_invis": "psnr_invis", "PSNR_vis": "psnr_vis", "SSIM": "ssim", "SSIM_invis": "ssim_invis",
         "SSIM_vis": "ssim_vis", "PercSim": "percsim", "PercSim_invis": "percsim_invis", "PercSim_vis": "percsim_vis"}
ALL_COLUMNS = COLUMNS + PERCSIM_COLUMNS     # the rows' columns with --vgg16


def discover(pred, gt, sampled=None, max_img=None):
    """-> list of (pred_path, gt_path, sampled_path or None) for i = 0, 1, ...  Raises FileNotFoundError naming what is missing."""
    dirs = [pred, gt] + ([sampled] if sampled else [])
    if max_img is None:
        n = 0
        while os.path.exists(os.path.join(pred, f"{n}.png")):
            n += 1
    else:
        n = int(max_img)
        if n < 0:
            raise ValueError(f"--max-img must be >= 0, got {n}")
    missing = [os.path.join(d, f"{i}.png") for i in range(n) for d in dirs if not os.path.exists(os.path.join(d, f"{i}.png"))]
    if missing:
        raise FileNotFoundError(f"{len(missing)} image(s) missing, first: {missing[:3]}")
    return [(os.path.join(pred, f"{i}.png"), os.path.join(gt, f"{i}.png"),
             os.path.join(sampled, f"{i}.png") if sampled else None) for i in range(n)]


def _threads():
    env = os.environ.get("OMP_NUM_THREADS")
    n = int(env) if env and env.isdigit() and int(env) > 0 else (os.cpu_count() or 1)
    return max(1, min(16, n))


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im if im.mode == "RGB" else im.convert("RGB"), dtype=np.uint8)


def _decode(item):
    """-> (pred (H, W, 3) u8, gt (H, W, 3) u8, vis mask (H, W) f32 or None)"""
    p, g, s = item
    pred, gt = _read_rgb(p), _read_rgb(g)
    if pred.shape != gt.shape:
        raise ValueError(f"{p} and {g} differ in size: {pred.shape} vs {gt.shape}")
    mask = None
    if s is not None:
        smp = _read_rgb(s)
        if smp.shape != gt.shape:
            raise ValueError(f"{s} and {g} differ in size: {smp.shape} vs {gt.shape}")
        mask = np.all(gt == smp, axis=2).astype(np.float32)
    return pred, gt, mask


def _pinned(arrays):
    return torch.from_numpy(np.stack(arrays)).pin_memory()


def _stage(decoded):
    """decoded images of one batch -> pinned host tensors (pred, gt (B, H, W, 3) u8; mask (B, 1, H, W) f32 or None)"""
    shapes = {d[0].shape for d in decoded}
    if len(shapes) != 1:
        raise ValueError(f"images of one batch differ in size: {sorted(shapes)} (use --batch 1)")
    mask = None if decoded[0][2] is None else _pinned([d[2][None] for d in decoded])
    return _pinned([d[0] for d in decoded]), _pinned([d[1] for d in decoded]), mask


def _score_batches(items, batch, pool, decode, score, width):
    """The loop of both modes: `decode` runs on the host pool one batch of items ahead of the device; score(items of the batch, what
    decode gave for each) stages them pinned, uploads and scores them -> a (len, width) device tensor, read back with the batch's one
    synchronisation.  -> (len(items), width) float64 rows, in order"""
    own = pool is None
    pool = pool or ThreadPoolExecutor(max_workers=_threads())
    try:
        chunks = [items[i:i + batch] for i in range(0, len(items), batch)]
        submit = lambda ch: [pool.submit(decode, it) for it in ch]
        rows = []
        pending = submit(chunks[0]) if chunks else None
        for k, chunk in enumerate(chunks):
            decoded = [f.result() for f in pending]
            pending = submit(chunks[k + 1]) if k + 1 < len(chunks) else None     # decodes while the device scores this batch
            rows.append(score(chunk, decoded).cpu().double().numpy())            # the batch's one synchronisation
        return np.concatenate(rows) if rows else np.zeros((0, width))
    finally:
        if own:
            pool.shutdown()


def score_files(items, device, batch=64, pool=None, pnet=None, inception=None):
    """-> (len(items), 6) float64 numpy rows (COLUMNS) of the (pred, gt, sampled) triples, in order; with a PNet `pnet`
    (len(items), 9) rows (ALL_COLUMNS).  With a FIDInception `inception`: -> (those rows, (len(items), 2 * 2048) float64 feature rows,
    the --pred image's features then the --gt image's)."""
    def score(_, decoded):
        pred, gt, mask = (None if t is None else t.to(device, non_blocking=True) for t in _stage(decoded))
        # (B, H, W, 3) storage read as (B, 3, H, W) through its strides: no copy
        out = image_metrics(gt.permute(0, 3, 1, 2), pred.permute(0, 3, 1, 2), mask)
        if pnet is not None:
            out = torch.cat([out, perceptual_rows(pnet, gt.permute(0, 3, 1, 2), pred.permute(0, 3, 1, 2), mask)], 1)
        if inception is not None:
            both = FID.inception_features(inception, torch.cat([pred, gt]).permute(0, 3, 1, 2))
            out = torch.cat([out, both[:len(pred)], both[len(pred):]], 1)
        return out
    k = 6 if pnet is None else len(ALL_COLUMNS)
    out = _score_batches(items, batch, pool, _decode, score, k + (0 if inception is None else 2 * FID.I.DIMS))
    if inception is None:
        return out
    return np.ascontiguousarray(out[:, :k]), np.ascontiguousarray(out[:, k:])


def summarize(rows, masked, percsim=False):
    """-> {printed name: mean over images} in the reference's print order (utils/calc_errors.py:93-101); percsim: rows carry
    ALL_COLUMNS"""
    names = ["PSNR", "PSNR_invis", "PSNR_vis", "SSIM", "SSIM_invis", "SSIM_vis"] if masked else ["PSNR", "SSIM"]
    if percsim:
        names += ["PercSim", "PercSim_invis", "PercSim_vis"] if masked else ["PercSim"]
    out = {}
    for name in names:
        col = rows[:, ALL_COLUMNS.index(NAMES[name])].astype(np.float32)     # the reference averages float32 results
        if name.startswith("PSNR"):
            col = np.minimum(col, np.float32(PSNR_CLAMP))
        out[name] = float(np.mean([float(v) for v in col])) if len(col) else float("nan")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pred", help="directory of predicted <i>.png")
    ap.add_argument("--gt", help="directory of ground-truth <i>.png")
    ap.add_argument("--sampled", help="directory of the sampled images: adds the vis / invis split")
    ap.add_argument("--max-img", type=int, help="score i < N (default: as long as --pred has <i>.png)")
    ap.add_argument("--batch", type=int, default=64, help="images per upload and launch")
    ap.add_argument("--json", help="write per-image rows and the means here")
    ap.add_argument("--vgg16", help="VGG16 weights (vgg16-397923af.pth or a PNet state dict): adds PercSim")
    ap.add_argument("--inception", help="Inception-v3 weights (pt_inception-2015-12-05-*.pth or a state dict with torchvision's keys): "
                                        "adds FID of --pred against --gt")
    ap.add_argument("--consistency", help="homography consistency mode: directory of the view pairs <%%04d>/output_image_<d>_000{1,2}.png")
    ap.add_argument("--masks", help="with --consistency: directory of <%%04d>/mask1.png, mask2.png")
    ap.add_argument("--points", help="with --consistency: directory of reproj1_<i>.npy, reproj2_<i>.npy")
    ap.add_argument("--directions", help="with --consistency: .npy of each item's direction index into consistency.MAPPING")
    args = ap.parse_args(argv)
    if args.consistency is None:
        missing = [o for o, v in (("--pred", args.pred), ("--gt", args.gt)) if v is None]
        if missing:
            ap.error("the following arguments are required: " + ", ".join(missing))
        stray = [o for o, v in (("--masks", args.masks), ("--points", args.points), ("--directions", args.directions)) if v is not None]
        if stray:
            ap.error(f"{', '.join(stray)} go with --consistency")
    else:
        missing = [o for o, v in (("--masks", args.masks), ("--points", args.points), ("--directions", args.directions)) if v is None]
        if missing:
            ap.error("--consistency requires " + ", ".join(missing))
        stray = [o for o, v in (("--pred", args.pred), ("--gt", args.gt), ("--sampled", args.sampled), ("--inception", args.inception))
                 if v is not None]
        if stray:
            ap.error(f"{', '.join(stray)} do not go with --consistency")
    if args.batch < 1:
        ap.error("--batch must be >= 1")
    if args.vgg16 is not None and not os.path.isfile(args.vgg16):
        ap.error(f"--vgg16 {args.vgg16}: no such file")
    if args.inception is not None and not os.path.isfile(args.inception):
        ap.error(f"--inception {args.inception}: no such file")
    if args.consistency is not None:
        return _consistency_main(args)

    masked = args.sampled is not None

    def items():
        found = discover(args.pred, args.gt, args.sampled, args.max_img)
        if args.inception is not None and len(found) < 2:
            raise SystemExit(f"--inception: FID needs two images at least, found {len(found)}")
        return found

    def score(mine, device, pnet):
        net = None
        if args.inception is not None:
            from .networks.inception import FIDInception
            net = FIDInception(weights=args.inception, use_gpu=True)
        local = score_files(mine, device, args.batch, pnet=pnet, inception=net)
        # the feature rows travel with the metric rows: float64 blocks, fp32 features pass unchanged
        return local if net is None else np.concatenate(local, 1)

    def means_of(rows, percsim):
        means = summarize(rows, masked, percsim)
        if args.inception is not None:
            feats = rows[:, -2 * FID.I.DIMS:]
            means["FID"] = FID.fid_of_rows(feats[:, :FID.I.DIMS], feats[:, FID.I.DIMS:])
        return means

    def columns(percsim):
        cols = COLUMNS if masked else ("psnr", "ssim")
        if percsim:
            cols = cols + (PERCSIM_COLUMNS if masked else ("percsim",))
        return [(c, ALL_COLUMNS.index(c)) for c in cols]
    return _run(args, ("pred", "gt", "sampled"), items, score, means_of, columns)


def _run(args, named, discover_items, score, means_of, columns):
    """What both modes do around their scoring: set up, deal the items over the ranks, score this rank's (score(items, device, pnet)
    -> (len, k) rows), gather every rank's rows in item order and, on rank 0, print means_of(rows, percsim) and write --json: n, the
    arguments `named`, the means and per item the columns(percsim) = [(name, column of rows)]."""
    rank, world, device = _setup()
    try:
        items = discover_items()
        n = len(items)
        mine = D.shard_views(n, rank, world)
        pnet = None
        if args.vgg16 is not None:
            from .networks.pretrained_networks import PNet
            pnet = PNet(use_gpu=True, weights=args.vgg16)
        rows = D.gather_rows(score([items[i] for i in mine], device, pnet).T, n).T          # (n, k), item order
        if rank == 0:
            means = means_of(rows, pnet is not None)
            for name, v in means.items():
                print("%s \t %0.5f" % (name, v))
            if args.json:
                doc = {"n": n, **{k: getattr(args, k) for k in named}, "psnr_clamp": PSNR_CLAMP, "means": means,
                       **({"fid": means["FID"]} if "FID" in means else {}),
                       "rows": [dict(index=i, **{c: float(rows[i, j]) for c, j in columns(pnet is not None)}) for i in range(n)]}
                with open(args.json, "w") as fh:
                    json.dump(doc, fh, indent=1)
    finally:
        if world > 1:
            torch.distributed.destroy_process_group()
    return 0


def _setup():
    """-> (rank, world size, device): the device of this rank, and the process group when there is more than one rank"""
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = 0 if os.environ.get("PS_DRYRUN_ONE_GPU") == "1" else int(os.environ.get("LOCAL_RANK", 0))
    if not torch.cuda.is_available():
        raise SystemExit("pixelsynth_amd.evaluate needs the ROCm device (there is no CPU fallback)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("PS_DRYRUN_ONE_GPU") == "1":
            torch.distributed.init_process_group("gloo")
        else:
            torch.distributed.init_process_group("nccl", device_id=device)
    return rank, world, device


# ---- the homography consistency mode (calc_errors_consistency_homography.py)
CONSISTENCY_SIZE = 256                       # the reference's 255 literals and (256, 256, 1) reshapes


def consistency_discover(views, masks, points, directions, max_img=None):
    """-> list of (index, view1, view2, mask1, mask2, reproj1, reproj2) paths for i < len(directions) (or < max_img).  Raises
    FileNotFoundError naming the first missing file, ValueError for a direction outside consistency.MAPPING."""
    dirs = np.load(directions)
    if dirs.ndim != 1:
        raise ValueError(f"{directions}: a 1-D array of direction indices expected, got shape {dirs.shape}")
    n = len(dirs) if max_img is None else int(max_img)
    if n < 0:
        raise ValueError(f"--max-img must be >= 0, got {n}")
    if n > len(dirs):
        raise ValueError(f"--max-img {n}: {directions} holds {len(dirs)} directions")
    out = []
    for i in range(n):
        d = int(dirs[i])
        if not 0 <= d < len(CS.MAPPING):
            raise ValueError(f"{directions}: item {i}: direction {d} outside 0 .. {len(CS.MAPPING) - 1}")
        item = (i, os.path.join(views, "%04d" % i, "output_image_%s_0001.png" % CS.MAPPING[d]),
                os.path.join(views, "%04d" % i, "output_image_%s_0002.png" % CS.MAPPING[d]),
                os.path.join(masks, "%04d" % i, "mask1.png"), os.path.join(masks, "%04d" % i, "mask2.png"),
                os.path.join(points, "reproj1_%d.npy" % i), os.path.join(points, "reproj2_%d.npy" % i))
        for p in item[1:]:
            if not os.path.exists(p):
                raise FileNotFoundError(f"item {i}: {p} is missing")
        out.append(item)
    return out


def _read_gray(path):
    """ImageOps.grayscale(Image.open(path)) as (H, W) uint8: PIL's integer L conversion"""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        return np.asarray(ImageOps.grayscale(im), dtype=np.uint8)


def _decode_item(item):
    """-> (view1, view2 (H, W, 3) u8, mask1, mask2 (H, W) u8, reproj1, reproj2)"""
    i, v1, v2, m1, m2, p1, p2 = item
    arrs = (_read_rgb(v1), _read_rgb(v2), _read_gray(m1), _read_gray(m2))
    S = CONSISTENCY_SIZE
    for path, a in zip((v1, v2, m1, m2), arrs):
        if a.shape[:2] != (S, S):
            raise ValueError(f"item {i}: {path} is {a.shape[1]} x {a.shape[0]}; the consistency score takes {S} x {S} frames")
    pts = []
    for path in (p1, p2):
        p = np.load(path)
        if p.ndim != 2 or p.shape[1] < 2 or p.dtype.kind not in "iuf":
            raise ValueError(f"item {i}: {path} holds a {p.dtype} array of shape {p.shape}; (n, >= 2) real numbers expected")
        pts.append(p)
    return arrs + tuple(pts)


def consistency_files(items, device, batch=64, pool=None, pnet=None):
    """-> (len(items), 3) float64 rows (consistency.COLUMNS[:3]), or (len(items), 6) with a PNet, in order"""
    def score(chunk, dec):
        H12, H21 = CS.fit_points([d[4] for d in dec], [d[5] for d in dec], [it[0] for it in chunk])
        v1, v2, m1, m2 = (_pinned([d[j] for d in dec]).to(device, non_blocking=True) for j in range(4))
        return CS.consistency_rows(v1.permute(0, 3, 1, 2), v2.permute(0, 3, 1, 2), m1[:, None], m2[:, None], H12, H21, pnet=pnet)
    return _score_batches(items, batch, pool, _decode_item, score, 3 if pnet is None else 6)


def consistency_summarize(rows, percsim=False):
    """-> {printed name: mean over items} in the reference's METRICS order (PercSim_vis, PSNR_vis): per item
    (dir0 + dir1) * 0.5 of the fp32 per-direction values in fp64, then np.mean (:103-109)"""
    out = {}
    for name, c0 in ((("PercSim_vis", 3),) if percsim else ()) + (("PSNR_vis", 0),):
        d0, d1 = rows[:, c0].astype(np.float32), rows[:, c0 + 1].astype(np.float32)
        per = [(float(a) + float(b)) * .5 for a, b in zip(d0, d1)]
        out[name] = float(np.mean(per)) if per else float("nan")
    return out


def _consistency_main(args):
    k = 3 if args.vgg16 is None else 6
    return _run(args, ("consistency", "masks", "points", "directions"),
                lambda: consistency_discover(args.consistency, args.masks, args.points, args.directions, args.max_img),
                lambda mine, device, pnet: consistency_files(mine, device, args.batch, pnet=pnet).reshape(-1, k),
                consistency_summarize, lambda percsim: [(c, j) for j, c in enumerate(CS.COLUMNS[:k])])


if __name__ == "__main__":
    raise SystemExit(main())
