"""Score predicted views against ground truth: PSNR and SSIM on the HIP kernel (csrc/metrics.hip) and, with --vgg16, PercSim (the
VGG16 perceptual similarity, perceptual.py); the reference's calc_errors_quality.py without FID (it needs Inception weights).

    python -m pixelsynth_amd.evaluate --pred DIR --gt DIR [--sampled DIR] [--max-img N] [--batch 64] [--json PATH] [--vgg16 PATH]

Image i is <dir>/<i>.png in each directory.  Without --max-img, i runs from 0 as long as --pred has <i>.png; with it, every i < N must be
there.  Images are read as RGB.  With --sampled, a pixel is "vis" where all channels of the ground truth equal the sampled image
(calc_errors_quality.py:28-35), which adds PSNR_vis / PSNR_invis and SSIM_vis / SSIM_invis.  One line per metric, its mean over the
images (PSNR clamped at 100 first, as the reference does).  --json writes the per-image rows and the means.  --vgg16 names VGG16
weights (torchvision's vgg16-397923af.pth, or a PNet state dict; nothing is downloaded) and adds PercSim -- with --sampled also
PercSim_invis and PercSim_vis, the images times the mask -- after the SSIM lines, means of the per-image values (no clamp).

PNGs are decoded on a host thread pool (at most 16 threads), uploaded as pinned uint8 batches and scored on uint8 (the kernel converts
x / 255, TF.to_tensor's values); the next batch decodes while the device scores this one, one synchronisation per batch.  Under
torch.distributed.run the images are dealt with distributed.shard_views and the rows come back to every rank through one all-gather
(distributed.gather_rows); rank 0 prints and writes.  PS_DRYRUN_ONE_GPU=1 runs every rank on cuda:0 over gloo.
"""
import argparse
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import distributed as D
from .image_metrics import COLUMNS, image_metrics
from .perceptual import COLUMNS as PERCSIM_COLUMNS, perceptual_rows

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


def _stage(decoded):
    """decoded images of one batch -> pinned host tensors (pred, gt (B, H, W, 3) u8; mask (B, 1, H, W) f32 or None)"""
    shapes = {d[0].shape for d in decoded}
    if len(shapes) != 1:
        raise ValueError(f"images of one batch differ in size: {sorted(shapes)} (use --batch 1)")
    pred = torch.from_numpy(np.stack([d[0] for d in decoded])).pin_memory()
    gt = torch.from_numpy(np.stack([d[1] for d in decoded])).pin_memory()
    mask = None
    if decoded[0][2] is not None:
        mask = torch.from_numpy(np.stack([d[2] for d in decoded])[:, None]).pin_memory()
    return pred, gt, mask


def score_files(items, device, batch=64, pool=None, pnet=None):
    """-> (len(items), 6) float64 numpy rows (COLUMNS) of the (pred, gt, sampled) triples, in order; with a PNet `pnet`
    (len(items), 9) rows (ALL_COLUMNS)."""
    own = pool is None
    pool = pool or ThreadPoolExecutor(max_workers=_threads())
    try:
        chunks = [items[i:i + batch] for i in range(0, len(items), batch)]
        submit = lambda ch: [pool.submit(_decode, it) for it in ch]
        rows = []
        pending = submit(chunks[0]) if chunks else None
        for k in range(len(chunks)):
            host = _stage([f.result() for f in pending])
            pending = submit(chunks[k + 1]) if k + 1 < len(chunks) else None     # decodes while the device scores this batch
            pred, gt, mask = (None if t is None else t.to(device, non_blocking=True) for t in host)
            # (B, H, W, 3) storage read as (B, 3, H, W) through its strides: no copy
            out = image_metrics(gt.permute(0, 3, 1, 2), pred.permute(0, 3, 1, 2), mask)
            if pnet is not None:
                out = torch.cat([out, perceptual_rows(pnet, gt.permute(0, 3, 1, 2), pred.permute(0, 3, 1, 2), mask)], 1)
            rows.append(out.cpu().double().numpy())                               # the batch's one synchronisation
        return np.concatenate(rows) if rows else np.zeros((0, 6 if pnet is None else len(ALL_COLUMNS)))
    finally:
        if own:
            pool.shutdown()


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
    ap.add_argument("--pred", required=True, help="directory of predicted <i>.png")
    ap.add_argument("--gt", required=True, help="directory of ground-truth <i>.png")
    ap.add_argument("--sampled", help="directory of the sampled images: adds the vis / invis split")
    ap.add_argument("--max-img", type=int, help="score i < N (default: as long as --pred has <i>.png)")
    ap.add_argument("--batch", type=int, default=64, help="images per upload and launch")
    ap.add_argument("--json", help="write per-image rows and the means here")
    ap.add_argument("--vgg16", help="VGG16 weights (vgg16-397923af.pth or a PNet state dict): adds PercSim")
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be >= 1")
    if args.vgg16 is not None and not os.path.isfile(args.vgg16):
        ap.error(f"--vgg16 {args.vgg16}: no such file")

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
    try:
        items = discover(args.pred, args.gt, args.sampled, args.max_img)
        n = len(items)
        mine = D.shard_views(n, rank, world)
        pnet = None
        if args.vgg16 is not None:
            from .networks.pretrained_networks import PNet
            pnet = PNet(use_gpu=True, weights=args.vgg16)
        local_rows = score_files([items[i] for i in mine], device, args.batch, pnet=pnet)
        rows = D.gather_rows(local_rows.T, n).T                                    # (n, 6) -- 9 with --vgg16 --, image order
        masked = args.sampled is not None
        means = summarize(rows, masked, pnet is not None)
        if rank == 0:
            for name, v in means.items():
                print("%s \t %0.5f" % (name, v))
            if args.json:
                cols = COLUMNS if masked else ("psnr", "ssim")
                if pnet is not None:
                    cols = cols + (PERCSIM_COLUMNS if masked else ("percsim",))
                doc = {"n": n, "pred": args.pred, "gt": args.gt, "sampled": args.sampled, "psnr_clamp": PSNR_CLAMP, "means": means,
                       "rows": [dict(index=i, **{c: float(rows[i, ALL_COLUMNS.index(c)]) for c in cols}) for i in range(n)]}
                with open(args.json, "w") as fh:
                    json.dump(doc, fh, indent=1)
    finally:
        if world > 1:
            torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
