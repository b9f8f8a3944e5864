"""Soft z-buffer splatter on MI355X -- drop-in for the reference's
models/layers/z_buffer_layers.py:RasterizePointsXYsBlending (same constructor, same forward).

The reference rasterizes with PyTorch3D (rasterize_points + compositing.*, z_buffer_layers.py:81-84,
112-129) and materialises (B,S,S,K) idx/dist/alpha tensors; here one C-ABI call
(ps_splat_f32 -> pixelsynth_amd/csrc/splat.hip, its kernels in csrc/splat_pipeline.h) bins, sorts and composites on the fly.
There is no CPU fallback: tensors must live on the ROCm device.

Under autograd (grad mode on, pts3D or src requires grad) forward goes through _SplatFunction: the list-emitting route of ps_splat_f32
forward, ps_splat_backward_f32 (csrc/splat_bwd.hip, include/pixelsynth_splat_bwd.h) backward.
"""
import os
from collections import namedtuple

import torch
from torch import nn

from .. import _lib

ACCUMULATION = {"alphacomposite": 0, "wsum": 1, "wsumnorm": 2}


# radius_px, K, tau, rad_pow, accumulation, bg_ksize: the run of arguments every splat entry point takes, in the C ABI's order and types
SplatSettings = namedtuple("SplatSettings", "radius_px K tau rad_pow accumulation bg_ksize")

_WS = _lib.Workspace()         # the forward's scratch (the scene step's too: it is the forward's plus its block sums)
_WS_BWD = _lib.Workspace()     # the backward pass' two coefficient planes: kept apart, so that a forward between never regrows either


def splat_workspace(device, B, N, S, radius_px):
    return _WS.query(device, "ps_splat_workspace_bytes", B, N, S, float(radius_px))


def scene_workspace(device, B, cap, S, radius_px):
    return _WS.get(device, _lib.call("ps_scene_workspace_bytes", B, cap, S, float(radius_px)))


def splat_bwd_workspace(device, B, S, K):
    return _WS_BWD.query(device, "ps_splat_bwd_workspace_bytes", B, S, K)


class _SplatFunction(torch.autograd.Function):
    """(pts (B,N,3) f32 contiguous, feat (B,C,N) f32 contiguous, S, radius, K, tau, rad_pow, accumulation, bg_ksize) ->
    (features (B,C,S,S), background mask (B,S,S) uint8, not differentiable).  The caller's pts is left as it is: the negation is applied
    to a copy, which is saved with the K-nearest lists (idx int32 and dist f32, (B,S,S,K) each)."""

    @staticmethod
    def forward(ctx, pts, feat, S, radius, K, tau, rad_pow, accumulation, bg_ksize):
        B, N, C = pts.size(0), pts.size(1), feat.size(1)
        neg = pts.detach().clone()
        feat = feat.detach()
        out = torch.empty(B, C, S, S, dtype=torch.float32, device=pts.device)
        bg = torch.empty(B, S, S, dtype=torch.uint8, device=pts.device)
        idx = torch.empty(B, S, S, K, dtype=torch.int32, device=pts.device)
        dist = torch.empty(B, S, S, K, dtype=torch.float32, device=pts.device)
        ws = splat_workspace(pts.device, B, N, S, radius)
        _lib.call("ps_splat_f32", neg, feat, B, N, C, S, float(radius), K, float(tau), int(rad_pow), accumulation, int(bg_ksize),
                  out, bg, idx, None, dist, ws, ws.numel())
        ctx.save_for_backward(neg, feat, idx, dist)
        ctx.args = (B, N, C, S, float(radius), K, float(tau), int(rad_pow), accumulation)
        ctx.mark_non_differentiable(bg)
        return out, bg

    @staticmethod
    def backward(ctx, grad_out, _grad_bg):
        neg, feat, idx, dist = ctx.saved_tensors
        B, N, C, S, radius, K, tau, rad_pow, accumulation = ctx.args
        want_pts, want_feat = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_pts or want_feat):
            return (None,) * 9
        g = grad_out.float().contiguous()
        grad_pts = torch.empty_like(neg) if want_pts else None
        grad_feat = torch.empty_like(feat) if want_feat else None
        ws = splat_bwd_workspace(neg.device, B, S, K)
        _lib.call("ps_splat_backward_f32", neg, feat, idx, dist, g, B, N, C, S, radius, K, tau, rad_pow, accumulation,
                  grad_pts, grad_feat, ws, ws.numel())
        return (grad_pts, grad_feat) + (None,) * 7


class RasterizePointsXYsBlending(nn.Module):
    """Same inputs/outputs as the reference class (z_buffer_layers.py:12-131).

    forward(pts3D (B,N,3), src (B,C,N)) -> (features (B,C,S,S) f32, background_mask (B,S,S) bool).
    Like the reference, x and y of the caller's pts3D are negated in place (:71-72).

    The differentiable route.  With grad mode on and pts3D or src requiring grad (and return_debug False), the features carry a grad_fn
    and backward() gives gradients to src and to x and y of pts3D (z gets exact zeros: the z order is piecewise constant, as in
    PyTorch3D); background_mask is marked non-differentiable.  Its forward is the list-emitting route of ps_splat_f32: all K hits of
    every pixel, bit-exact lists -- so its features are those of return_debug=True, not the early-out product route's (which stops a
    pixel's walk once its transmittance is below 2^-23 and fuses the sum).  It saves the K-nearest lists for the backward pass: an
    int32 index and an fp32 distance per hit, 8 K bytes per pixel -- 67 MB per 256 x 256 frame at K = 128.  On this route the
    caller's pts3D is NOT negated in place, the one deviation from the reference's side effect: an in-place write into a tensor
    autograd tracks either raises (a leaf that requires grad) or invalidates what upstream nodes saved.  A call in which nothing
    requires grad, or one under torch.no_grad(), takes the route it always took, side effect included.  At the clamp of
    dist / r^rad_pow to [1e-3, 1] the gradient with respect to the points is exactly 0 where the clamp holds (bounds included)."""

    def __init__(self, C=64, learn_feature=True, radius=1.5, size=256, points_per_pixel=8, opts=None):
        super().__init__()
        # `default_feature` is never used by forward (in the reference neither) but checkpoints carry it:
        # a (1,C,1) parameter when learnt, a zero buffer otherwise
        if learn_feature:
            self.default_feature = nn.Parameter(torch.randn(1, C, 1))
        else:
            self.register_buffer("default_feature", torch.zeros(1, C, 1))
        self.radius, self.size, self.points_per_pixel, self.opts = radius, size, points_per_pixel, opts

    def _opt(self, name, default):
        return getattr(self.opts, name, default) if self.opts is not None else default

    def kernel_settings(self):
        """What the kernels take from this module and its opts, with the reference's defaults (z_buffer_layers.py:12-53)"""
        return SplatSettings(float(self.radius), int(self.points_per_pixel), float(self._opt("tau", 1.0)), int(self._opt("rad_pow", 2)),
                             ACCUMULATION[self._opt("accumulation", "alphacomposite")],
                             int(self._opt("background_smoothing_kernel_size", 13)))

    def forward(self, pts3D, src, return_debug=False):
        if src.dim() > 3:    # image-shaped input: (B,C,w,w) features with a (B,3,N) cloud, one row of points per w
            bs, c, w = src.shape[:3]
            image_size = w
            pts3D = pts3D.permute(0, 2, 1)
            src = src.unsqueeze(2).expand(bs, c, w, *src.shape[2:]).reshape(bs, c, -1)
        else:
            bs, image_size = src.size(0), self.size
        # cloud and features must be arranged alike: (B,N,3) against (B,C,N)
        if pts3D.size(2) != 3 or pts3D.size(1) != src.size(2):
            raise AssertionError(f"splat: points {tuple(pts3D.shape)} do not match features {tuple(src.shape)}")
        os.environ.get("DEBUG")  # the reference reads os.environ["DEBUG"] (KeyError if unset); tolerated here

        B, N, C = bs, pts3D.size(1), src.size(1)
        if not return_debug and torch.is_grad_enabled() and (pts3D.requires_grad or src.requires_grad):
            out, bg = _SplatFunction.apply(pts3D.float().contiguous(), src.float().contiguous(), int(image_size), *self.kernel_settings())
            return out, bg.view(torch.bool)
        caller_pts = pts3D
        pts = pts3D if (pts3D.is_contiguous() and pts3D.dtype == torch.float32) else pts3D.float().contiguous()
        feat = src.float().contiguous()
        S = int(image_size)
        K = int(self.points_per_pixel)
        out = torch.empty(B, C, S, S, dtype=torch.float32, device=pts.device)
        bg = torch.empty(B, S, S, dtype=torch.uint8, device=pts.device)
        idx = zbuf = dist = None
        if return_debug:
            idx = torch.empty(B, S, S, K, dtype=torch.int32, device=pts.device)
            zbuf = torch.empty(B, S, S, K, dtype=torch.float32, device=pts.device)
            dist = torch.empty(B, S, S, K, dtype=torch.float32, device=pts.device)
        ws = splat_workspace(pts.device, B, N, S, self.radius)
        _lib.call("ps_splat_f32", pts, feat, B, N, C, S, *self.kernel_settings(), out, bg, idx, zbuf, dist, ws, ws.numel())
        if pts is not caller_pts:  # keep the reference's visible side effect on the caller's tensor
            caller_pts[:, :, 0:2] = pts[:, :, 0:2].to(caller_pts.dtype)
        background_mask = bg.view(torch.bool)    # (k_dilate writes 0 / 1: the same bytes are the boolean mask)
        if return_debug:
            return out, background_mask, idx, zbuf, dist
        return out, background_mask
