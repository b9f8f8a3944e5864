"""GPU: the prefix pass with the dependency cone as EXACT sets (k_prefix_sets, tuning value prefix_exact) and with every product
stage walking a list of its own evaluated items (k_perm_compact, prefix_compact) -- lmconv_plan.hip.

What is pinned: (a) the device's bit sets equal oracle/prefix_cone_oracle.exact_need_sets for every stage and frame, with per-frame
prefix ends; (b) the per-(stage, share) lists are the sorted lists filtered in order and their lengths are the sets' popcounts;
(c) codes and the logits of the walked locations are bit-identical whatever the two switches say, for 0 / 1 masks, fractional masks
and two frame ranges on two streams; (d) a pipelined handle whose caches hold other batches' rows gives the codes of fresh handles
(rows a stage skips keep old values: nothing may read them); (e) ps_pixelcnn_status is clean after each."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, prefix_cone_oracle as pc
from pixelsynth_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["right_half", "half_plus_island", "ragged", "top_band"]
SETTINGS = [dict(prefix_full=1, prefix_exact=1, prefix_compact=1), dict(prefix_full=0, prefix_exact=0, prefix_compact=0),
            dict(prefix_full=0, prefix_exact=1, prefix_compact=0), dict(prefix_full=0, prefix_exact=0, prefix_compact=1),
            dict(prefix_full=0, prefix_exact=1, prefix_compact=1)]
DEFAULTS = dict(prefix_full=0, prefix_exact=1, prefix_compact=1, prefix_cone_force=0, gemm_merge_min=8192, gemm_wg_min=256,
                gemm_ws_min=1024, gemm_ws=7)


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_net(seed=0):
    from pixelsynth_amd.lmconv.layers import PONO
    from pixelsynth_amd.lmconv.model import OurPixelCNN
    net = OurPixelCNN(nr_resnet=2, nr_filters=80, input_channels=512, nr_logistic_mix=10, kernel_size=(3, 3), max_dilation=2,
                      weight_norm=False, feature_norm_op=lambda _c: PONO(), dropout_prob=0, conv_bias=True, conv_mask_weight=False,
                      rematerialize=False, binarize=False).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(seed).items()}, strict=True)
    return net.to(DEV)


def make_model():
    import types
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts
    o = dict(W=256, use_rgb_features=True, splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=128, tau=1.0,
             rad_pow=2, accumulation="alphacomposite", background_smoothing_kernel_size=13, min_z=1.0, max_z=100.0,
             rotation=0.6, direction="R", temperature=0.7, model_setting="gen_img", seed=0, homography=False)
    m = ZbufferModelPts(types.SimpleNamespace(**o)).eval()
    m.outpaint2.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()})
    return m.to(DEV)


def fixture_frames(F_):
    bgs = syn.background_masks(256)
    infos = [c_oracle.masks_for_background(bgs[NAMES[b % 4]], 32) for b in range(F_)]
    order_loc = np.stack([(i["order"][:, 0] * 32 + i["order"][:, 1]) for i in infos]).astype(np.int32)
    return infos, order_loc


def device_array(eng, idx, shape, typestr="<i4"):
    """A copy of one of the prefix pass's tables (ps_pixelcnn_debug_cache selector 10) on the host."""
    from pixelsynth_amd import _lib
    ptr = _lib.call("ps_pixelcnn_debug_cache", eng.handle, 10, idx)
    assert ptr
    raw = type("Raw", (), {"__cuda_array_interface__": {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}})()
    torch.cuda.synchronize()
    return torch.as_tensor(raw, device=DEV).clone().cpu().numpy()


def pack_bits(sets, words):
    """(npre,) bool by rank -> (words,) uint32, bit r & 31 of word r >> 5."""
    full = np.zeros(words * 32, bool)
    full[:len(sets)] = sets
    return np.packbits(full, bitorder="little").view("<u4")


@pytest.mark.parametrize("F_,first", [(16, 480), (5, 700)])   # (16 frames: one share per XCD; 5: one share)
def test_device_sets_and_stage_lists_against_the_oracle(F_, first):
    """(a) + (b), on a batch with per-frame ends: frame f's prefix ends at first + 16 * (f % 3)."""
    infos, order_loc = fixture_frames(F_)
    net = make_net(5)
    eng = net.engine(32, 32, F_)
    ends = (first + 16 * (np.arange(F_) % 3)).astype(np.int32)
    npre = int(ends.max())
    reg = np.zeros((F_, 1024), np.uint8)
    for b in range(F_):
        reg[b, order_loc[b][ends[b]:]] = 1
    ms = [tt(np.concatenate([i[k] for i in infos])) for k in ("mask_init", "mask_undilated", "mask_dilated")]
    codes = tt(syn.codes(31, F_).reshape(F_, 1024).astype(np.int32))
    eng.set_tuning(gemm_merge_min=0, gemm_wg_min=1, gemm_ws_min=1, gemm_ws=7)
    eng.ar_prefix(codes, tt(order_loc), tt(reg), *ms, first, 0, F_, first_steps=tt(ends), max_first_step=npre)
    eng.check()
    bits = device_array(eng, 0, (pc.N_EVAL, F_, 32), "<u4")
    want_cache = {}
    fewer = 0
    for b in range(F_):
        key = (b % 4, int(ends[b]))
        if key not in want_cache:
            o = order_loc[b].astype(np.int64)
            und, dil = infos[b]["mask_undilated"][0], infos[b]["mask_dilated"][0]
            want_cache[key] = (pc.exact_need_sets(o, und, dil, 32, 32, int(ends[b])), pc.prefix_starts(o, und, dil, 32, 32, int(ends[b])))
        sets, starts = want_cache[key]
        for s in range(pc.N_EVAL):
            assert np.array_equal(bits[s, b], pack_bits(sets[s], 32)), (s, b)
            assert not sets[s][:starts[s]].any()                       # (the exact set lies inside the suffix the start rank keeps)
            fewer += int(ends[b]) - int(starts[s]) - int(sets[s].sum())
    assert fewer > 0                                                    # exactness removes something
    # (b) the stages' own lists
    parts = 8 if F_ >= 16 and F_ % 8 == 0 else 1
    share_len = (F_ // parts) * npre if parts > 1 else F_ * npre
    cnt = device_array(eng, 1, (pc.N_EVAL - 1, F_))
    lists = device_array(eng, 2, (pc.N_EVAL - 1, F_ * 1024, 2))
    sorted_lists = device_array(eng, 3, (2, F_ * 1024, 2))
    for s in range(1, pc.N_EVAL):
        src = sorted_lists[1 if s >= 29 else 0]
        total = 0
        for sh in range(parts):
            run = src[sh * share_len:(sh + 1) * share_len]
            fl, r = run[:, 0] // npre, run[:, 0] % npre
            assert fl.min() >= sh * (F_ // parts) and fl.max() < (sh + 1) * (F_ // parts) if parts > 1 else True
            keep = ((bits[s, fl, r >> 5] >> (r & 31).astype(np.uint32)) & 1).astype(bool)
            n = int(cnt[s - 1, sh])
            assert n == int(keep.sum()), (s, sh)
            assert np.array_equal(lists[s - 1, sh * share_len:sh * share_len + n], run[keep]), (s, sh)
            total += n
        assert total == sum(bin(int(w)).count("1") for w in bits[s].ravel()), s
    eng.set_tuning(**DEFAULTS)
    eng.check()


def _ar_case(F_, first, fractional):
    from pixelsynth_amd.lmconv.model import wavefronts
    infos, order_loc = fixture_frames(F_)
    reg = np.zeros((F_, 1024), np.uint8)
    rs = np.random.RandomState(F_)
    for b in range(F_):
        walked = order_loc[b][first:]
        reg[b, walked[rs.rand(walked.size) < 0.7]] = 1
        reg[b, order_loc[b][first]] = 1
    masks = [np.concatenate([i[k] for i in infos]).copy() for k in ("mask_init", "mask_undilated", "mask_dilated")]
    if fractional:   # a third of the open taps of every other frame get a value that is neither 0 nor 1 (open stays open) -- at the
        # locations in front of `first` in the frame's order, the ones the prefix pass evaluates: a walked location's type-B values
        # must stay 0 / 1 (include/pixelsynth_hip.h at ps_pixelcnn_ar_run)
        prefix = np.zeros((F_, 1, 1024), bool)
        for b in range(1, F_, 2):
            prefix[b, 0, order_loc[b][:first]] = True
        for m_ in masks[1:]:
            scale = np.where(prefix & (rs.rand(*m_.shape) < 0.33), 0.25 + 0.5 * rs.rand(*m_.shape), 1.0).astype(np.float32)
            open_ = prefix & (m_ > 0)
            m_ *= scale
            assert (m_[open_] != 1.0).mean() > 0.2          # (the case cannot silently become a 0 / 1 case)
    ms = [tt(m_) for m_ in masks]
    codes0 = syn.codes(23, F_).reshape(F_, 1024).astype(np.int32)
    u = tt(np.random.RandomState(5).rand(F_, 1024).astype(np.float32))
    return order_loc, reg, ms, codes0, u, wavefronts(order_loc, 32, 32, first, DEV)


@pytest.mark.parametrize("F_,first,fractional", [(16, 500, False), (7, 600, False), (16, 640, True), (3, 905, True)])
def test_switches_change_no_bit(F_, first, fractional):
    """(c) on one stream: prefix_full, neither switch, each alone, both -- the same codes and the same logits at every walked location."""
    order_loc, reg, ms, codes0, u, waves = _ar_case(F_, first, fractional)
    eng = make_net(5).engine(32, 32, F_)
    eng.set_tuning(prefix_cone_force=1, gemm_merge_min=0, gemm_wg_min=1, gemm_ws_min=1, gemm_ws=7)
    walked = np.zeros((F_, 1024), bool)
    for b in range(F_):
        walked[b, order_loc[b][first:]] = True
    sel = torch.from_numpy(walked).to(DEV)
    out = []
    n0 = eng.launch_counts()
    for cfg in SETTINGS:
        eng.set_tuning(**cfg)
        c = tt(codes0.copy())
        lg = eng.ar_run(c, tt(order_loc), tt(reg), *ms, temperature=0.7, uniforms=u, first_step=first, want_logits=True, waves=waves)
        eng.check()
        out.append((c, lg[sel].clone()))
    n1 = eng.launch_counts()
    assert n1["k_gemm_ws<0>"] - n0["k_gemm_ws<0>"] == 14 * len(SETTINGS)    # (the form that reads the stages' lists is the one that ran)
    eng.set_tuning(**DEFAULTS)
    for cfg, (c, lg) in zip(SETTINGS[1:], out[1:]):
        assert torch.equal(c, out[0][0]), cfg
        assert torch.equal(lg, out[0][1]), cfg
    assert (out[0][0].cpu().numpy()[reg == 1] != codes0[reg == 1]).any()


def test_switches_change_no_bit_over_two_frame_ranges_on_two_streams():
    """(c) with the pass dealt to two frame ranges on two streams (one of 16 frames: a share per XCD; one of 21: one share), each range
    with its own part of the sets, the lists and their counts."""
    from pixelsynth_amd.lmconv.model import CuRangeStream
    F_, first, cut = 37, 700, 16
    order_loc, reg, ms, codes0, u, waves = _ar_case(F_, first, False)
    eng = make_net(3).engine(32, 32, F_)
    eng.set_tuning(gemm_merge_min=0, gemm_wg_min=1, gemm_ws_min=1, gemm_ws=7)
    o, r = tt(order_loc), tt(reg)
    A, B = CuRangeStream(0, 160), CuRangeStream(160, 96)
    eng.set_compute_units(160)
    got = []
    for cfg in SETTINGS:
        eng.set_tuning(**cfg)
        c = tt(codes0.copy())
        torch.cuda.synchronize()
        with torch.cuda.stream(B.stream):
            eng.ar_prefix(c, o, r, *ms, first, 0, cut)
            done = torch.cuda.Event()
            done.record(B.stream)
        with torch.cuda.stream(A.stream):
            eng.ar_prefix(c, o, r, *ms, first, cut, F_)
            A.stream.wait_event(done)
            eng.ar_columns(c, o, r, *ms, waves, temperature=0.7, uniforms=u, first_step=first)
        A.stream.synchronize()
        eng.check()
        got.append(c)
    eng.set_compute_units(0)
    eng.set_tuning(**DEFAULTS)
    for cfg, c in zip(SETTINGS[1:], got[1:]):
        assert torch.equal(c, got[0]), cfg
    assert (got[0].cpu().numpy()[reg == 1] != codes0[reg == 1]).any()


def test_a_pipelined_handle_full_of_other_batches_rows_gives_the_codes_of_fresh_handles():
    """(d) Three different batches of 16 views through one pipelined handle, four in flight, twice round (every quarter of the handle
    is reused by another batch, whose skipped rows still hold the earlier batch's values), against each batch alone in a handle that has
    seen nothing else."""
    V = 16
    cam = syn.demo_cameras(V)
    K, Kinv, P, Pinv = (tt(cam[k]) for k in ("K", "Kinv", "P", "Pinv"))
    batches = []
    for b in range(3):
        img, depth = tt(syn.image(681 + b, V, 3, 256)), tt(syn.depth_smooth(691 + b, V, 256, 1.0, 100.0))
        yaws = np.linspace(-0.7 + 0.1 * b, 0.5 + 0.1 * b, V)
        rts = [syn.yaw_pose(cam["P"][v:v + 1], float(y)) for v, y in enumerate(yaws)]
        RT2, RT2inv = tt(np.concatenate([x[1] for x in rts])), tt(np.concatenate([x[0] for x in rts]))
        batches.append(((img, depth, K, Kinv, P, Pinv, RT2, RT2inv), tt(syn.codes(701 + b, V)), tt(np.random.RandomState(711 + b).rand(V, 1024).astype(np.float32))))
    ref = []
    for a, c, u in batches:
        fresh = make_model()
        ref.append(fresh.outpaint_planned(fresh.plan_views(*a), c, temperature=0.7, uniforms=u)["codes"].clone())
        fresh.outpaint2.engine(32, 32, V).check()
        del fresh
    assert not torch.equal(ref[0], ref[1]) and not torch.equal(ref[1], ref[2])
    m = make_model()
    assert m.pipe_depth(V) == 4
    eng = m.outpaint2.engine(32, 32, m.pipe_frames(V))
    eng.set_tuning(gemm_merge_min=0, gemm_wg_min=1, gemm_ws_min=1, gemm_ws=7)      # (16 views: the form that reads the stages' lists)
    assert eng.get_tuning("prefix_exact") == 1 and eng.get_tuning("prefix_compact") == 1
    got = []
    for k in range(6):
        a, c, u = batches[k % 3]
        done = m.outpaint_pipelined(m.plan_views(*a), c, temperature=0.7, uniforms=u)
        if done is not None:
            got.append(done["codes"].clone())
    got += [o["codes"].clone() for o in m.outpaint_flush()]
    torch.cuda.synchronize()
    eng.check()
    eng.set_tuning(**{k: v for k, v in DEFAULTS.items() if k.startswith("gemm")})
    assert len(got) == 6
    for k in range(6):
        assert torch.equal(got[k], ref[k % 3]), (k, int((got[k] != ref[k % 3]).sum()))
