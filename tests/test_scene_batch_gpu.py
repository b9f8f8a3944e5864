"""GPU tests of the batched chained-scene path: B independent scenes advance one frame per step together on ragged clouds that stay on
the device (csrc/scene.hip, PtsManipulator.forward_scene_step, ZbufferModelPts.forward_scene with B > 1).

Bar: scene b of a batch is the B = 1 route's result BIT FOR BIT (torch.equal) -- features, background mask, cloud, kept features, every
output of forward_scene; against the C oracle the mask is exact and the features within the 1e-6 tests/test_splat_gpu.py states for the
product route."""
import types

import numpy as np
import pytest
import torch

from oracle import c_oracle
from pixelsynth_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _manip(W, K=128):
    from pixelsynth_amd.projection.z_buffer_manipulator import PtsManipulator
    o = types.SimpleNamespace(splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=K, tau=1.0, rad_pow=2,
                              accumulation="alphacomposite", background_smoothing_kernel_size=13)
    return PtsManipulator(W, C=3, opt=o).to(DEV)


def _state(B, C, cap):
    from pixelsynth_amd.projection.z_buffer_manipulator import SceneState
    return SceneState(B, C, cap, torch.device(DEV))


def _cameras(B):
    """demo cameras, every scene's source pose turned a little differently"""
    cam = syn.demo_cameras(B)
    for b in range(B):
        inv, rt = syn.yaw_pose(cam["P"][b:b + 1], 0.05 * b, 0.02 * b)
        cam["P"][b], cam["Pinv"][b] = rt[0], inv[0]
    return cam


def _poses(P, yaws):
    pairs = [syn.yaw_pose(P[b:b + 1], y) for b, y in enumerate(yaws)]
    return np.concatenate([p[1] for p in pairs]), np.concatenate([p[0] for p in pairs])   # RT, RTinv


def _chain(B, S, seed):
    """Three frames of B scenes: images, depths, per-scene poses, and the background masks that select frame 1's and frame 2's new
    points -- counts that differ per scene, among them a scene with no new point and one whose mask is all ones."""
    rs = np.random.RandomState(seed)
    cam = _cameras(B)
    frames = []
    for f in range(3):
        RT, RTinv = _poses(cam["P"], [0.3 + 0.15 * f - 0.1 * b for b in range(B)])
        mask = None
        if f:
            mask = rs.rand(B, S, S) < rs.uniform(0.1, 0.6, (B, 1, 1))
            mask[(f - 1) % B] = False          # no new point
            mask[f % B] = True                 # every pixel new
            mask[(f + 1) % B, : S // 3] = True
        frames.append(dict(img=syn.image(seed + 10 * f, B, 3, S), depth=syn.depth_uniform(seed + 10 * f + 1, B, S, 1.0, 100.0),
                           RT=RT, RTinv=RTinv, mask=mask))
    return cam, frames


def _run_both(pm, cam, frames, B, S, cap, after_step=None):
    """The batched route on one state against forward_justpts_cumulative on every scene alone; torch.equal after every step."""
    st = _state(B, 3, cap)
    K, Kinv = tt(cam["K"]), tt(cam["Kinv"])
    single = [dict(cloud=None, src=None) for _ in range(B)]
    RT1, RT1inv = tt(cam["P"]), tt(cam["Pinv"])
    prev_RTinv, counts = None, [0] * B
    for f, fr in enumerate(frames):
        img, depth, RT2, RT2inv = tt(fr["img"]), tt(fr["depth"]), tt(fr["RT"]), tt(fr["RTinv"])
        mask = None if fr["mask"] is None else tt(fr["mask"])
        feat, bg = pm.forward_scene_step(st, img, depth, K, Kinv, RT1, RT1inv, RT2, RT2inv, mask, prev_RTinv)
        counts = [S * S] * B if mask is None else [c + int(fr["mask"][b].sum()) for b, c in enumerate(counts)]
        assert st.counts == counts and st.count.cpu().tolist() == counts, f"frame {f}: counts {st.counts} / {st.count.cpu().tolist()}, host {counts}"
        assert mask is None or len(set(counts)) > 1     # ragged: the scenes' clouds differ in length
        for b in range(B):
            sl = slice(b, b + 1)
            r = pm.forward_justpts_cumulative(img[sl], depth[sl], K[sl], Kinv[sl], RT1[sl], RT1inv[sl], RT2[sl], RT2inv[sl],
                                              single[b]["cloud"], single[b]["src"], None if mask is None else mask[sl],
                                              None if prev_RTinv is None else prev_RTinv[sl])
            f1, bg1, cloud1, src1 = r
            assert torch.equal(bg[b], bg1[0]), f"frame {f} scene {b}: background mask"
            assert torch.equal(feat[b], f1[0]), f"frame {f} scene {b}: features, max |d| = {(feat[b] - f1[0]).abs().max().item():.3g}"
            assert torch.equal(st.cloud[b, :, :counts[b]], cloud1[0]), f"frame {f} scene {b}: cloud"
            assert torch.equal(st.feats[b, :, :counts[b]], src1[0]), f"frame {f} scene {b}: kept features"
            single[b] = dict(cloud=cloud1, src=src1)
        if after_step is not None:
            after_step(f, fr, feat, bg, single)
        RT1, RT1inv, prev_RTinv = RT2, RT2inv, RT2inv
    return st


@pytest.mark.parametrize("S,K", [(64, 32), (256, 128)])
def test_ragged_step_equals_the_per_scene_step_bit_for_bit(S, K):
    """Frame 0, then two chained frames of B = 4 scenes with different images, depths, poses and numbers of new points: after every
    step scene b's features, background mask, cloud[b, :, :count[b]] and kept features are torch.equal to forward_justpts_cumulative
    on that scene alone (the existing route, itself oracle-tested in tests/test_splat_gpu.py), and count equals the host's
    bookkeeping."""
    B = 4
    cam, frames = _chain(B, S, seed=40 + S)
    _run_both(_manip(S, K), cam, frames, B, S, cap=3 * S * S)


def test_ragged_step_against_the_c_oracle():
    """Every scene of a chained batched step against the C oracle called once per scene at B = 1 (the committed oracle handles equal
    counts only): background mask exact, features within the 1e-6 tests/test_splat_gpu.py states for the product route."""
    B, S, K = 4, 64, 32
    cam, frames = _chain(B, S, seed=7)
    ref_cloud, ref_src, checked = [None] * B, [None] * B, []

    def oracle(f, fr, feat, bg, single):
        RT1inv = cam["Pinv"] if f == 0 else frames[f - 1]["RTinv"]
        for b in range(B):
            sl = slice(b, b + 1)
            img, depth = fr["img"][sl].reshape(1, 3, -1), fr["depth"][sl]
            if f == 0:
                s, c = c_oracle.project_pts_cumulative(depth, None, None, cam["K"][sl], cam["Kinv"][sl], RT1inv[sl], fr["RT"][sl], None, S)
                src = img
            else:
                m = fr["mask"][sl].reshape(1, -1)
                s, c = c_oracle.project_pts_cumulative(depth.reshape(1, -1)[m].reshape(1, 1, -1), m, ref_cloud[b], cam["K"][sl],
                                                       cam["Kinv"][sl], RT1inv[sl], fr["RT"][sl], frames[f - 1]["RTinv"][sl], S)
                src = np.concatenate([img[:, :, m[0]], ref_src[b]], axis=2)
            ref = c_oracle.splat_forward(np.ascontiguousarray(s.transpose(0, 2, 1)), np.ascontiguousarray(src), S, K=K)
            assert np.array_equal(single[b]["cloud"].cpu().numpy(), c)
            assert np.array_equal(bg[b].cpu().numpy(), ref["bg"][0]), f"frame {f} scene {b}"
            np.testing.assert_allclose(feat[b].cpu().numpy(), ref["feat"][0], rtol=0, atol=1e-6, err_msg=f"frame {f} scene {b}")
            ref_cloud[b], ref_src[b] = c, src
            checked.append((f, b))

    _run_both(_manip(S, K), cam, frames, B, S, cap=3 * S * S, after_step=oracle)
    assert len(checked) == 3 * B


def test_first_batched_step_equals_the_unchained_path():
    """No mask, no prior: the first step of B scenes is forward_justpts on the same batch, features and mask, bit for bit (the
    shipped configuration: 256 x 256, K = 128, r = 4)."""
    B, S = 3, 256
    cam, frames = _chain(B, S, seed=3)
    fr = frames[0]
    pm = _manip(S)
    args = [tt(a) for a in (fr["img"], fr["depth"], cam["K"], cam["Kinv"], cam["P"], cam["Pinv"], fr["RT"], fr["RTinv"])]
    st = _state(B, 3, S * S)
    feat, bg = pm.forward_scene_step(st, *args)
    f0, bg0 = pm.forward_justpts(*args)
    assert torch.equal(bg, bg0) and torch.equal(feat, f0)
    assert st.counts == [S * S] * B and st.count.cpu().tolist() == [S * S] * B
    assert 0.02 < bg.float().mean().item() < 0.98


def test_a_step_that_does_not_fit_is_refused_on_the_host_and_names_the_scene():
    """cap one point too small for the second frame: the step raises before the launch (the check is host bookkeeping: nothing runs
    out of bounds to provoke it), names the scene, and leaves the state as it was -- the same state, grown to a sufficient cap,
    carries on and gives the per-scene route's bits."""
    B, S, K = 3, 64, 32
    cam, frames = _chain(B, S, seed=11)
    pm = _manip(S, K)
    need = [S * S + int(frames[1]["mask"][b].sum()) for b in range(B)]
    worst = int(np.argmax(need))
    st = _state(B, 3, max(need) - 1)
    K_, Kinv = tt(cam["K"]), tt(cam["Kinv"])
    f0 = frames[0]
    pm.forward_scene_step(st, tt(f0["img"]), tt(f0["depth"]), K_, Kinv, tt(cam["P"]), tt(cam["Pinv"]), tt(f0["RT"]), tt(f0["RTinv"]))
    before = (st.counts[:], st.count.clone(), st.cloud.clone(), st.feats.clone())
    f1 = frames[1]
    step1 = lambda s: pm.forward_scene_step(s, tt(f1["img"]), tt(f1["depth"]), K_, Kinv, tt(f0["RT"]), tt(f0["RTinv"]), tt(f1["RT"]),
                                            tt(f1["RTinv"]), tt(f1["mask"]), tt(f0["RTinv"]))
    with pytest.raises(RuntimeError, match=rf"scene {worst} would hold {max(need)} points.*cap = {max(need) - 1}"):
        step1(st)
    assert st.counts == before[0] and torch.equal(st.count, before[1])
    assert torch.equal(st.cloud, before[2]) and torch.equal(st.feats, before[3])
    big = st.grown(max(need))
    feat, bg = step1(big)
    assert big.counts == need and big.count.cpu().tolist() == need
    ref = _state(B, 3, 3 * S * S)
    pm.forward_scene_step(ref, tt(f0["img"]), tt(f0["depth"]), K_, Kinv, tt(cam["P"]), tt(cam["Pinv"]), tt(f0["RT"]), tt(f0["RTinv"]))
    feat_r, bg_r = step1(ref)
    assert torch.equal(feat, feat_r) and torch.equal(bg, bg_r)
    for b in range(B):
        assert torch.equal(big.cloud[b, :, :need[b]], ref.cloud[b, :, :need[b]])
        assert torch.equal(big.feats[b, :, :need[b]], ref.feats[b, :, :need[b]])
    # the library's own last line of defence: a next_max past cap is an argument error, nothing is enqueued
    from pixelsynth_amd import _lib
    assert _lib.call("ps_scene_state_bytes", B, 3, big.cap) == big.nbytes
    assert _lib.call("ps_scene_workspace_bytes", 0, 10, 16, 4.0) == 0


# ---------------------------------------------------------------------------------------------- forward_scene
def _scene_model(**kw):
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts
    o = dict(W=256, use_rgb_features=True, splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=128, tau=1.0,
             rad_pow=2, accumulation="alphacomposite", background_smoothing_kernel_size=13, min_z=1.0, max_z=100.0,
             rotation=0.6, direction="R", temperature=0.7, seed=0, homography=False, vqvae=True, model_setting="gen_scene",
             num_split=2, directions=["R", "L"], num_samples=1, sequential_outpainting=False)
    o.update(kw)
    m = ZbufferModelPts(types.SimpleNamespace(**o)).eval()
    m.outpaint2.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()})
    m.vqvae.load_state_dict({k: torch.from_numpy(v) for k, v in syn.vqvae_state_dict(0).items()}, strict=True)
    return m.to(DEV).eval()


def _scene_batch(B, directions=None):
    cam = {k: torch.from_numpy(v) for k, v in _cameras(B).items()}
    # noise over a low-frequency pattern of the scene's own: depth_from_image (a box filter of the luminance) differs from scene to scene
    img = (0.3 * syn.image(31, B, 3, 256) + 0.7 * syn.depth_smooth(32, B, 256, -1.0, 1.0)).astype(np.float32)
    batch = {"images": [torch.from_numpy(img)], "cameras": [cam], "depth_fn": syn.depth_from_image}
    if directions is not None:
        batch["direction"] = torch.tensor(directions)
    return batch


def _one(batch, b):
    out = {"images": [batch["images"][0][b:b + 1]], "cameras": [{k: v[b:b + 1] for k, v in batch["cameras"][0].items()}],
           "depth_fn": batch["depth_fn"]}
    if "direction" in batch:
        out["direction"] = batch["direction"][b:b + 1]
    return out


def _assert_slices_equal(m, batch, B, want_keys, ragged):
    _, out = m(batch)
    m.outpaint2.engine(32, 32, B).check()
    counts = set()
    for b in range(B):
        _, one = m(_one(batch, b))
        m.outpaint2.engine(32, 32, 1).check()
        assert want_keys(b) <= set(one), sorted(want_keys(b) - set(one))
        for k, v in one.items():
            assert k in out, k
            assert tuple(out[k].shape) == (B,) + tuple(v.shape[1:]), (k, tuple(out[k].shape), tuple(v.shape))
            assert torch.equal(out[k][b:b + 1], v), f"scene {b}: {k}, max |d| = {(out[k][b:b + 1].float() - v.float()).abs().max().item():.3g}"
        counts.add(int((one[sorted(k for k in one if k.startswith('ForegroundImg'))[0]] == 0).sum()))
    assert not ragged or len(counts) > 1, "the scenes' clouds should differ in length"
    return out


@pytest.mark.parametrize("sequential", [False, True])
def test_forward_scene_batch_equals_every_scene_alone(sequential):
    """gen_scene, B = 3, directions R then L, num_split = 2: slice b of every output is torch.equal to the B = 1 run of scene b (same
    poses, same draws, same pictures), and the engine's status is clean.  (The poses of a sweep are rotations about the camera centre:
    what they disocclude does not depend on the depth, so these scenes' clouds grow alike; clouds of different lengths are the per-scene
    directions of the next test and the masks of the step tests above.)"""
    m = _scene_model(sequential_outpainting=sequential)
    keys = {f"{kind}_{d}_{i}" for kind in ("PredImg", "FeaturesImg") for d in ("R", "L") for i in range(3)}
    keys |= {f"{kind}_{d}_2" for kind in ("PredDepthImg", "ForegroundImg") for d in ("R", "L")} | {"InputImg"}
    out = _assert_slices_equal(m, _scene_batch(3), 3, lambda b: keys, ragged=False)
    assert set(out) == keys
    assert tuple(out["ForegroundImg_R_2"].shape) == (3, 1, 256, 256) and tuple(out["PredImg_L_0"].shape) == (3, 3, 256, 256)


def test_gen_two_imgs_batch_with_per_scene_directions():
    """gen_two_imgs, B = 4, every scene in a direction of its own (indices 0, 1, 2, 5 of the reference's mapping): scene b's slice
    under ITS direction's keys is the B = 1 run of scene b."""
    m = _scene_model(model_setting="gen_two_imgs")
    dirs = [0, 1, 2, 5]
    names = [m.mapping[d] for d in dirs]
    want = lambda b: {f"PredImg_{names[b]}_{i}" for i in range(3)} | {f"ForegroundImg_{names[b]}_2", "InputImg"}
    out = _assert_slices_equal(m, _scene_batch(4, dirs), 4, want, ragged=True)
    assert {f"PredImg_{n}_1" for n in names} | {f"PredImg_{n}_2" for n in names} <= set(out)


def test_forward_scene_batch_refuses_what_it_cannot_do():
    m = _scene_model(model_setting="gen_two_imgs")
    batch = _scene_batch(2, [0, 1, 2])
    with pytest.raises(ValueError, match=r"2 images need a \(B,\) direction, got 3"):
        m(batch)
    m.opt.num_samples = 2
    with pytest.raises(NotImplementedError, match="num_samples"):
        m(_scene_batch(2, [0, 1]))
