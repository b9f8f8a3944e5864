"""Inputs and host-side references the CPU and GPU tests of the device ranking route share (test_rank_device_cpu.py,
test_rank_device_gpu.py)."""
import numpy as np
import torch
from PIL import Image

SIZES = [(256, 224), (32, 28), (20, 33), (16, 16)]


def byte_images(S, seed=0):
    """uint8 (S,S,3): random, saturated, and a 0/255 checkerboard (per pixel and channel)"""
    rng = np.random.default_rng(seed)
    yy, xx, cc = np.meshgrid(np.arange(S), np.arange(S), np.arange(3), indexing="ij")
    return {"random": rng.integers(0, 256, (S, S, 3), dtype=np.uint8), "all255": np.full((S, S, 3), 255, np.uint8),
            "checker": (((yy + xx + cc) & 1) * 255).astype(np.uint8)}


def floats_of_bytes(raw):
    """fp32 in [-1,1] that the host's quantisation turns into `raw`: the middle of every byte's bucket (255: exactly 1)"""
    x = np.minimum((raw.astype(np.float64) + 0.5) / 255.0 * 2.0 - 1.0, 1.0).astype(np.float32)
    assert np.array_equal(((x * .5 + .5) * 255).astype(np.uint8), raw)
    return x


def host_lines(img, T):
    """_entropy_score's numpy lines (z_buffermodel.py) on one (3,S,S) fp32 candidate, for any S and T -> (input (3,T,T), bytes (T,T,3))"""
    S = img.shape[-1]
    raw = ((img.reshape([S, S, 3]) * .5 + .5) * 255).astype(np.uint8)
    resized = np.asarray(Image.fromarray(raw).resize((T, T), Image.BILINEAR))
    im = np.asarray(resized, np.float32) / 255.0
    im = (im - np.array([0.485, 0.456, 0.406], np.float32)) / np.array([0.229, 0.224, 0.225], np.float32)
    return torch.from_numpy(im).permute(2, 0, 1).contiguous().numpy(), resized


def score_lists(n, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(n).astype(np.float32) * 0.37 - 3.0, rng.permutation(n).astype(np.float32) * 0.11 + 1.0   # distinct


def select_cases():
    """(disc, entr) lists for the rank rule: distinct scores for n in 1, 2, 3, 17, 50, 64, and the same with one NaN in either list"""
    cases = []
    for n in (1, 2, 3, 17, 50, 64):
        for seed in range(2):
            disc, entr = score_lists(n, seed)
            cases.append((disc, entr))
            for which in range(2 if n > 1 else 0):
                lists = [disc.copy(), entr.copy()]
                lists[which][(seed + 1) % n] = np.nan
                cases.append(tuple(lists))
    return cases


def input_images(S):
    """fp32 (3,3,S,S) for the classifier-input kernel.  Read as (S,S,3) pictures: 0 is noise whose edge rows and columns are +-1 (the
    clipped 2-tap outputs of the resample see other values than the interior); 1 is noise with every quantisation threshold
    2k/255 - 1 laid into it, each with its two fp32 neighbours, and exact +-1, +-0; 2 is plain noise."""
    rng = np.random.default_rng(S)
    imgs = rng.uniform(-1, 1, (3, 3, S, S)).astype(np.float32)
    edge = imgs[0].reshape(S, S, 3)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = 1.0, -1.0, -1.0, 1.0
    t = (2.0 * np.arange(256) / 255.0 - 1.0).astype(np.float32)
    t = np.concatenate([np.nextafter(t, np.float32(-2)), t, np.nextafter(t, np.float32(2)), np.float32([1, -1, 0, -0.0])])
    t = np.clip(t, -1, 1)[rng.permutation(len(t))]
    flat = imgs[1].reshape(-1)
    count = min(len(t), len(flat) // 2)
    flat[rng.choice(len(flat), count, replace=False)] = t[:count]
    return imgs
