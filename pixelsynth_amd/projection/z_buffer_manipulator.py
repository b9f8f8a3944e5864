"""Point-cloud reprojection on MI355X -- drop-in for the reference's
models/projection/z_buffer_manipulator.py:PtsManipulator (same constructor and method signatures).

project_pts / project_pts_cumulative run in csrc/splat.hip:k_project through the C ABI
(ps_project_pts_f32, ps_project_pts_cumulative_f32); forward_justpts uses the fused
ps_project_splat_f32 so the (B,N,3) cloud never leaves the scratch buffer.

Under autograd (grad mode on and the depth or the features requiring grad) project_pts is differentiable in the depth
(ps_project_pts_backward_f32, csrc/splat_bwd.hip) and forward_justpts in src and pred_pts: it then takes the unfused route, project_pts
and the splatter's differentiable route.  No gradient is produced for the camera matrices.  forward_justpts_cumulative /
project_pts_cumulative and forward_scene_step stay forward-only.

forward_scene_step advances B independent chained scenes by one frame on a SceneState -- per-scene clouds of different lengths that
stay on the device between frames (csrc/scene.hip through ps_scene_step_f32, include/pixelsynth_scene.h).
"""
import torch
import torch.nn as nn

from .. import _lib
from ..layers.z_buffer_layers import RasterizePointsXYsBlending, scene_workspace, splat_workspace

EPS = 1e-2


def get_splatter(name, depth_values, opt=None, size=256, C=64, points_per_pixel=8):
    """z_buffer_manipulator.py:11-27."""
    if name == "xyblending":
        return RasterizePointsXYsBlending(C, learn_feature=opt.learn_default_feature, radius=opt.radius,
                                          size=size, points_per_pixel=points_per_pixel, opts=opt)
    raise NotImplementedError()


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


class _ProjectFunction(torch.autograd.Function):
    """depth (B,N) f32 contiguous, cameras (B,4,4) f32 contiguous -> sampler (B,3,N); differentiable in the depth alone"""

    @staticmethod
    def forward(ctx, depth, K, K_inv, RTinv_cam1, RT_cam2, W):
        B = depth.size(0)
        out = torch.empty(B, 3, W * W, dtype=torch.float32, device=depth.device)
        _lib.call("ps_project_pts_f32", depth, K, K_inv, RTinv_cam1, RT_cam2, B, W, out)
        ctx.save_for_backward(depth, K, K_inv, RTinv_cam1, RT_cam2)
        ctx.W = W
        return out

    @staticmethod
    def backward(ctx, grad_sampler):
        depth, K, K_inv, RTinv_cam1, RT_cam2 = ctx.saved_tensors
        grad_depth = torch.empty_like(depth)
        _lib.call("ps_project_pts_backward_f32", depth, K, K_inv, RTinv_cam1, RT_cam2, grad_sampler.float().contiguous(),
                  depth.size(0), ctx.W, grad_depth)
        return grad_depth, None, None, None, None, None     # (no gradient for the camera matrices)


class SceneState:
    """The accumulated point clouds of B independent chained scenes (include/pixelsynth_scene.h): a ping-pong pair of homogeneous
    clouds (B,4,cap) and of their features (B,C,cap), the per-scene counts on the device (count (B) int32) and on the host (counts: the
    bookkeeping every step is checked against before anything is enqueued).  Logical point i of scene b is column i: the last frame's
    new points first, in row-major order of its mask, then the older cloud in its order (reference :248-266)."""

    def __init__(self, B, C, cap, device):
        self.B, self.C, self.cap = int(B), int(C), int(cap)
        if self.B <= 0 or self.C <= 0 or self.cap <= 0:
            raise ValueError(f"SceneState: B, C, cap must be positive (got {B}, {C}, {cap})")
        self._cloud = torch.empty(2, self.B, 4, self.cap, dtype=torch.float32, device=device)
        self._feat = torch.empty(2, self.B, self.C, self.cap, dtype=torch.float32, device=device)
        self.count = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.counts = [0] * self.B
        self._cur = 0
        assert self.nbytes == _lib.call("ps_scene_state_bytes", self.B, self.C, self.cap)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self._cloud, self._feat, self.count))

    @property
    def cloud(self):
        """(B,4,cap); scene b's points are cloud[b, :, :counts[b]]."""
        return self._cloud[self._cur]

    @property
    def feats(self):
        """(B,C,cap); scene b's features are feats[b, :, :counts[b]]."""
        return self._feat[self._cur]

    def reset(self):
        """Forget every scene's cloud (the next step is a first frame)."""
        self.counts = [0] * self.B
        self.count.zero_()

    def grown(self, cap):
        """A state of capacity `cap` >= this one's with the same contents (a copy on the device)."""
        if cap < max(self.counts):
            raise ValueError(f"SceneState.grown: cap {cap} < the {max(self.counts)} points a scene already holds")
        st = SceneState(self.B, self.C, cap, self.count.device)
        n = min(self.cap, cap)
        st._cloud[0, :, :, :n] = self.cloud[:, :, :n]
        st._feat[0, :, :, :n] = self.feats[:, :, :n]
        st.count.copy_(self.count)
        st.counts = list(self.counts)
        return st


class PtsManipulator(nn.Module):
    def __init__(self, W, C=64, opt=None):
        super().__init__()
        self.opt = opt
        self.W = W
        self.splatter = get_splatter(opt.splatter, None, opt, size=W, C=C, points_per_pixel=opt.pp_pixel)
        # the reference's `xyzs` buffer (:38-48) is kept so that state_dicts line up -- rows (x, -y, -1, 1) of the
        # align-corners NDC grid, row-major; the kernels regenerate these values on the fly
        axis = torch.arange(W, dtype=torch.float32) / float(W - 1) * 2 - 1
        gx = axis.view(1, W).expand(W, W).reshape(-1)
        gy = axis.view(W, 1).expand(W, W).reshape(-1)
        one = torch.ones(W * W)
        self.register_buffer("xyzs", torch.stack((gx, -gy, -one, one)).unsqueeze(0))

    # ------------------------------------------------------------------ a2
    def project_pts(self, pts3D, K, K_inv, RT_cam1, RTinv_cam1, RT_cam2, RTinv_cam2):
        """Reference :50-83.  pts3D (B,1,N) depth -> sampler (B,3,N); differentiable in the depth (not in the cameras)."""
        B = pts3D.size(0)
        N = self.W * self.W
        assert pts3D.numel() == B * N, "project_pts expects one depth per grid point"
        if torch.is_grad_enabled() and pts3D.requires_grad:
            return _ProjectFunction.apply(pts3D.float().contiguous().view(B, N), _f32c(K).detach(), _f32c(K_inv).detach(),
                                          _f32c(RTinv_cam1).detach(), _f32c(RT_cam2).detach(), self.W)
        depth = _f32c(pts3D)
        out = torch.empty(B, 3, N, dtype=torch.float32, device=depth.device)
        _lib.call("ps_project_pts_f32", depth, _f32c(K), _f32c(K_inv), _f32c(RTinv_cam1), _f32c(RT_cam2), B, self.W, out)
        return out

    # ------------------------------------------------------------------ a3
    def forward_justpts(self, src, pred_pts, K, K_inv, RT_cam1, RTinv_cam1, RT_cam2, RTinv_cam2):
        """Reference :85-107 -> (features (B,C,W,W), background_mask (B,W,W) bool).  With grad mode on and src or pred_pts requiring
        grad: the unfused route (project_pts, then the splatter), differentiable in both; else the fused call, as ever."""
        bs, c, w, h = src.size()
        differentiable = torch.is_grad_enabled() and (src.requires_grad or pred_pts.requires_grad)
        if len(pred_pts.size()) > 3 and w == self.W and h == self.W and not differentiable:
            sp = self.splatter
            S = self.W
            out = torch.empty(bs, c, S, S, dtype=torch.float32, device=src.device)
            bg = torch.empty(bs, S, S, dtype=torch.uint8, device=src.device)
            ws = splat_workspace(src.device, bs, S * S, S, sp.radius)
            _lib.call("ps_project_splat_f32", _f32c(pred_pts), _f32c(src), _f32c(K), _f32c(K_inv), _f32c(RTinv_cam1), _f32c(RT_cam2), bs, c, S,
                      *sp.kernel_settings(), out, bg, ws, ws.numel())
            return out, bg.view(torch.bool)    # (k_dilate writes 0 / 1: the same bytes are the boolean mask -- no conversion pass)
        if len(pred_pts.size()) > 3:
            pred_pts = pred_pts.view(bs, 1, -1)
            src = src.view(bs, c, -1)
        pts3D = self.project_pts(pred_pts, K, K_inv, RT_cam1, RTinv_cam1, RT_cam2, RTinv_cam2)
        pointcloud = pts3D.permute(0, 2, 1).contiguous()
        return self.splatter(pointcloud, src)

    # ------------------------------------------------------------------ a5
    def forward_justpts_cumulative(self, src1, pred_pts, K, K_inv, RT_cam1, RTinv_cam1, RT_cam2, RTinv_cam2,
                                   prior_point_cloud, src2, last_background_mask, RTinv_cam3):
        """Reference :184-219 -> (features, background_mask, new_point_cloud, src)."""
        bs, c = src1.shape[:2]
        mask_flat = None if last_background_mask is None else last_background_mask.view(bs, 1, -1)
        src = src1
        if pred_pts.dim() > 3:
            pred_pts = pred_pts.reshape(bs, 1, -1)
            src = src1.reshape(bs, c, -1)
            if src2 is not None:
                # only the points that fell on background last time are new; boolean gathers keep row-major order
                # (sized explicitly: a frame with no background at all contributes zero new points, where the
                # reference's view(bs, 1, -1) cannot infer a size)
                keep = mask_flat.bool()
                new_pts = pred_pts[keep]
                n_keep = new_pts.numel() // bs
                pred_pts = new_pts.view(bs, 1, n_keep)
                src = torch.cat([src[keep.expand(bs, c, -1)].view(bs, c, n_keep), src2.reshape(bs, c, -1)], dim=2)
        last_background_mask = mask_flat
        pts3D, new_point_cloud = self.project_pts_cumulative(
            pred_pts, K, K_inv, RT_cam1, RTinv_cam1, RT_cam2, RTinv_cam2, prior_point_cloud,
            last_background_mask, RTinv_cam3)
        pointcloud = pts3D.permute(0, 2, 1).contiguous()
        result, background_mask = self.splatter(pointcloud, src)
        return result, background_mask, new_point_cloud, src

    # ------------------------------------------------------------------ a4
    def project_pts_cumulative(self, pts3D, K, K_inv, RT_cam1, RTinv_cam1, RT_cam2, RTinv_cam2,
                               prior_point_cloud=None, last_background_mask=None, RTinv_cam3=None):
        """Reference :221-266 -> (sampler (B,3,NT), xy_proj (B,4,NT))."""
        B = pts3D.size(0)
        depth = _f32c(pts3D).view(B, pts3D.numel() // B)
        n_new = depth.size(1)
        new_index = None
        if last_background_mask is not None:
            m = last_background_mask.view(B, -1)
            # boolean-mask gather keeps row-major order (:226-228); equal counts per image as in the reference
            new_index = torch.nonzero(m, as_tuple=False)[:, 1].view(B, n_new).to(torch.int32).contiguous()
        n_prior = 0 if prior_point_cloud is None else prior_point_cloud.size(2)
        NT = n_new + n_prior
        sampler = torch.empty(B, 3, NT, dtype=torch.float32, device=depth.device)
        cloud = torch.empty(B, 4, NT, dtype=torch.float32, device=depth.device)
        prior = None if prior_point_cloud is None else _f32c(prior_point_cloud)
        rt3 = None if RTinv_cam3 is None else _f32c(RTinv_cam3)
        _lib.call("ps_project_pts_cumulative_f32", depth, new_index, prior, _f32c(K), _f32c(K_inv), _f32c(RTinv_cam1), _f32c(RT_cam2), rt3,
                  B, self.W, n_new, n_prior, sampler, cloud)
        return sampler, cloud

    # ------------------------------------------------------------------ a5 / a4 / a6, B scenes with ragged clouds
    def forward_scene_step(self, state, src, pred_pts, K, K_inv, RT_cam1, RTinv_cam1, RT_cam2, RTinv_cam2,
                           last_background_mask=None, RTinv_cam3=None, new_counts=None):
        """forward_justpts_cumulative for B independent scenes at once, on the state the scenes keep on the device:
        src (B,C,W,W) and pred_pts (B,1,W,W) of the frame rendered FROM, cameras (B,4,4); last_background_mask (B,W,W) bool and
        RTinv_cam3 of the previously rendered frame, both None for the first frame of the chains (every pixel a point, as
        forward_justpts; the state starts over).  -> (features (B,C,W,W), background_mask (B,W,W) bool); scene b's cloud and
        features are state.cloud[b, :, :state.counts[b]] and state.feats[b, :, :state.counts[b]] -- bit for bit what
        forward_justpts_cumulative returns for scene b alone.
        new_counts: the number of set pixels of every scene's mask where the caller already has them on the host (the AR plan
        reads the mask back: ARPlan.background_counts); otherwise they are read here (one copy of B integers).
        A step after which a scene would hold more than state.cap points raises before anything is enqueued and names the scene;
        the state is untouched."""
        sp, S = self.splatter, self.W
        B, C = src.shape[:2]
        if (B, C) != (state.B, state.C) or tuple(src.shape[2:]) != (S, S) or pred_pts.numel() != B * S * S:
            raise ValueError(f"forward_scene_step: src {tuple(src.shape)} / pred_pts {tuple(pred_pts.shape)} do not fit a state of "
                             f"{state.B} scenes with {state.C} features at W = {S}")
        first = last_background_mask is None
        if first:
            new_counts, prior = [S * S] * B, [0] * B
            mask = rt3 = None
        else:
            if RTinv_cam3 is None or min(state.counts) <= 0:
                raise ValueError("forward_scene_step: a chained frame needs RTinv_cam3 and a state that holds a first frame")
            mask = last_background_mask.reshape(B, S, S)
            mask = (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()
            if new_counts is None:
                new_counts = mask.view(B, -1).sum(1, dtype=torch.int32).tolist()
            prior, rt3 = state.counts, _f32c(RTinv_cam3)
        nxt = [int(p) + int(n) for p, n in zip(prior, new_counts)]
        over = [b for b in range(B) if nxt[b] > state.cap]
        if over:
            b = over[0]
            raise RuntimeError(f"forward_scene_step: scene {b} would hold {nxt[b]} points ({prior[b]} + {int(new_counts[b])} new), the "
                               f"state was created with cap = {state.cap}" + (f" (also scenes {over[1:]})" if over[1:] else ""))
        out = torch.empty(B, C, S, S, dtype=torch.float32, device=src.device)
        bg = torch.empty(B, S, S, dtype=torch.uint8, device=src.device)
        ws = scene_workspace(src.device, B, state.cap, S, sp.radius)
        cur, other = state._cur, 1 - state._cur
        _lib.call("ps_scene_step_f32", _f32c(pred_pts), _f32c(src), mask, state._cloud[cur], state._feat[cur], state._cloud[other],
                  state._feat[other], state.count, _f32c(K), _f32c(K_inv), _f32c(RTinv_cam1), _f32c(RT_cam2), rt3, B, C, S, state.cap,
                  max(prior), max(nxt), *sp.kernel_settings(), out, bg, ws, ws.numel())
        state._cur, state.counts = other, nxt
        return out, bg.view(torch.bool)
