"""Quality of rendered views (the reference's evaluation/, calc_errors_quality.py): PSNR and SSIM on the HIP kernel, and PercSim (the
VGG16 perceptual similarity: perceptual.py, networks/pretrained_networks.PNet) when the caller passes a PNet, overall and split into the
pixels the splat covered ("vis") and the outpainted ones ("invis").  The homography consistency score of view pairs
(calc_errors_consistency_homography.py: PSNR_vis and PercSim_vis of each view warped into the other's frame) is consistency_rows
(consistency.py).  FID (Inception weights, pytorch_fid) and LPIPS are not provided."""
from ..consistency import COLUMNS as CONSISTENCY_COLUMNS, consistency_rows
from ..image_metrics import COLUMNS, image_metrics
from ..perceptual import COLUMNS as PERCSIM_COLUMNS, perceptual_rows

__all__ = ["score_views", "consistency_rows", "COLUMNS", "PERCSIM_COLUMNS", "CONSISTENCY_COLUMNS"]


def score_views(pred, gt, background_mask=None, pnet=None):
    """pred, gt (B, 3, H, W) frames in the model's [-1, 1] space (mapped by 0.5 x + 0.5, as base_model.py:97-99 does before
    scoring); background_mask (B, H, W) bool, True where no point was splatted (outpaint_views / synthesize_views) -- "vis" is
    ~background_mask, "invis" the outpainted region.  -> dict of (B,) f32 tensors: psnr, ssim, and with a mask the vis / invis
    columns as well; with a PNet `pnet` also percsim (and with a mask percsim_vis / percsim_invis), the masked variants scoring the
    images times the mask as calc_errors_quality.py does."""
    a, b = pred * 0.5 + 0.5, gt * 0.5 + 0.5
    mask = None
    if background_mask is not None:
        if background_mask.dim() != 3 or tuple(background_mask.shape) != (pred.shape[0],) + tuple(pred.shape[2:]):
            raise ValueError(f"background_mask must be (B, H, W), got {tuple(background_mask.shape)} for frames {tuple(pred.shape)}")
        mask = (~background_mask.bool()).unsqueeze(1)
    rows = image_metrics(a, b, mask)
    keep = COLUMNS if mask is not None else ("psnr", "ssim")
    out = {k: rows[:, COLUMNS.index(k)] for k in keep}
    if pnet is not None:
        prow = perceptual_rows(pnet, a, b, mask)
        for k in PERCSIM_COLUMNS if mask is not None else ("percsim",):
            out[k] = prow[:, PERCSIM_COLUMNS.index(k)]
    return out
