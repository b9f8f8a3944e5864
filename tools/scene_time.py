"""Time chained scenes through the batched route (ZbufferModelPts.forward_scene with B > 1: ragged clouds kept on the device,
csrc/scene.hip) next to the B = 1 route called B times, for B in {1, 4, 16, 64}, on the MI355X.

    python tools/scene_time.py [--batches 1 4 16 64] [--iters 8]

A chain is TWO frames (gen_scene, one direction, num_split = 1: first the far end of the sweep, no prior; then the view back at the
source, rendered from the generated far end on top of its cloud) with everything of a frame in the loop: depth stand-in, reprojection
+ splat, AR plan, VQ-VAE codes, AR outpainting, decode, blend.  "splat" times the reprojection + splat of the same two frames alone (PtsManipulator.forward_scene_step
against forward_justpts_cumulative per scene, masks fixed), the part this route replaces.  The two routes ALTERNATE within the call,
after a warm-up of both (2 calls each); every sample is _measure.event_ms of work that ends in a synchronise; the figure is the median.
At B = 1 forward_scene takes the B = 1 route itself: both columns then time the same code, and their difference is the noise floor.

Prints one JSON line: ms per scene-frame per route and B, and the bytes of state and workspace per scene at the capacity used."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixelsynth_amd import _lib, synthetic as syn  # noqa: E402
from pixelsynth_amd.projection.z_buffer_manipulator import SceneState  # noqa: E402
from pixelsynth_amd.z_buffermodel import ZbufferModelPts  # noqa: E402
from _measure import event_ms  # noqa: E402

S, FRAMES = 256, 2


def make_model(dev):
    o = dict(W=S, use_rgb_features=True, splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=128, tau=1.0, rad_pow=2,
             accumulation="alphacomposite", background_smoothing_kernel_size=13, min_z=1.0, max_z=100.0, rotation=0.6, direction="R",
             temperature=0.7, seed=0, homography=False, vqvae=True, model_setting="gen_scene", num_split=1, directions=["R"],
             num_samples=1, sequential_outpainting=False)
    m = ZbufferModelPts(types.SimpleNamespace(**o)).eval()
    m.outpaint2.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()})
    m.vqvae.load_state_dict({k: torch.from_numpy(v) for k, v in syn.vqvae_state_dict(0).items()}, strict=True)
    return m.to(dev).eval()


def scenes(B, dev):
    img = (0.3 * syn.image(31, B, 3, S) + 0.7 * syn.depth_smooth(32, B, S, -1.0, 1.0)).astype(np.float32)
    cam = {k: torch.from_numpy(v).to(dev) for k, v in syn.demo_cameras(B).items()}
    return torch.from_numpy(img).to(dev), cam


def take_turns(batched, single, iters):
    for _ in range(2):
        batched()
        single()
    tb, ts = [], []
    for _ in range(iters):
        tb.append(event_ms(batched))
        ts.append(event_ms(single))
    return statistics.median(tb), statistics.median(ts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--iters", type=int, default=8)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    m = make_model(dev)
    pm = m.pts_transformer
    cap = m.SCENE_CAP_FRAMES * S * S
    out = {"size": S, "frames_per_chain": FRAMES, "iters": args.iters, "cap": cap,
           "state_bytes_per_scene": _lib.call("ps_scene_state_bytes", 1, 3, cap),
           "workspace_bytes_per_scene": _lib.call("ps_scene_workspace_bytes", 1, cap, S, 4.0), "B": {}}
    for B in args.batches:
        img, cam = scenes(B, dev)
        batch = {"images": [img], "cameras": [cam], "depth_fn": syn.depth_from_image}
        ones = [{"images": [img[b:b + 1]], "cameras": [{k: v[b:b + 1] for k, v in cam.items()}], "depth_fn": syn.depth_from_image}
                for b in range(B)]
        with torch.no_grad():
            _, ref = m(batch)
            for b in (0, B - 1):      # the two routes render the same pictures
                _, one = m(ones[b])
                assert all(torch.equal(ref[k][b:b + 1], v) for k, v in one.items()), f"B = {B}: scene {b} differs between the routes"

            def scene_batched():
                m(batch)
                torch.cuda.synchronize()

            def scene_single():
                for one in ones:
                    m(one)
                torch.cuda.synchronize()
            t_b, t_s = take_turns(scene_batched, scene_single, args.iters)

            # the reprojection + splat of the same two frames alone, on fixed inputs
            depth = syn.depth_from_image(img)
            RTinv, RT = (torch.cat(t) for t in zip(*[m.get_rt_from_rot("R", cam["P"][b:b + 1], 1, 1) for b in range(B)]))
            args0 = (img, depth, cam["K"], cam["Kinv"], cam["P"], cam["Pinv"], RT, RTinv)
            st = SceneState(B, 3, cap, dev)
            _, bg = pm.forward_scene_step(st, *args0)
            counts = bg.view(B, -1).sum(1, dtype=torch.int32).tolist()
            img1 = ref["PredImg_R_1"]
            args1 = (img1, syn.depth_from_image(img1), cam["K"], cam["Kinv"], RT, RTinv, cam["P"], cam["Pinv"])

            def splat_batched():
                pm.forward_scene_step(st, *args0)
                pm.forward_scene_step(st, *args1, bg, RTinv, new_counts=counts)
                torch.cuda.synchronize()

            def splat_single():
                for b in range(B):
                    sl = slice(b, b + 1)
                    r = pm.forward_justpts_cumulative(*[a[sl] for a in args0], None, None, None, None)
                    pm.forward_justpts_cumulative(*[a[sl] for a in args1], r[2], r[3], bg[sl], RTinv[sl])
                torch.cuda.synchronize()
            p_b, p_s = take_turns(splat_batched, splat_single, args.iters)
        per = 1.0 / (B * FRAMES)
        out["B"][str(B)] = {"batched_ms_per_scene_frame": round(t_b * per, 4), "b1_route_ms_per_scene_frame": round(t_s * per, 4),
                            "speedup": round(t_s / t_b, 2), "splat_batched_ms_per_scene_frame": round(p_b * per, 4),
                            "splat_b1_route_ms_per_scene_frame": round(p_s * per, 4), "splat_speedup": round(p_s / p_b, 2),
                            "points_per_scene_after_frame_1": [min(counts) + S * S, max(counts) + S * S]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
