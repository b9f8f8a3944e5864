"""GPU: mask values other than 0 / 1 through the PixelCNN engine (lmconv.hip, lmconv_grid.hip, lmconv_column.hip, lmconv_tp.hip).

The locally masked convolution multiplies the unfolded input by whatever the mask holds (locally_masked_convolution.py:24-27).  The
whole-grid pass honours that for all three masks (k_gemm loads the values; k_gemm_wg / k_gemm_ws load them for the items that
k_perm_scatter flags; u_init multiplies by the type-A values).  The column kernels do not: their neighbour role takes a type-B tap as
open or closed and their chain role the centre as open, so a location WALKED AS A COLUMN must carry type-B values that are exactly
0 / 1 with the centre 1 -- k_ctx_build refuses anything else (include/pixelsynth_hip.h at ps_pixelcnn_ar_run).

  (a) eng.forward with fractional values in all three masks: k_gemm, k_gemm_wg, k_gemm_ws and the unsorted item walk bit-equal, and
      each within BAR of the twin;
  (b) AR runs whose PREFIX locations carry fractional masks (the columns read cache rows computed under them; their own type-B values
      are 0 / 1), and, in one parameter, fractional TYPE-A values at the walked locations too: at every walked location the logits are
      the whole-grid pass's on the completed grid bit for bit, and within BAR of the twin -- walk, latency-form waves, both
      throughput-form kernels, and the split prefix / columns calls;
  (c) one offending type-B value at one walked location: ps_pixelcnn_status names mask values in every form, and the same handle then
      gives the bits of a fresh handle on 0 / 1 masks.  (To get there nothing leaves its bounds: k_ctx_build reads the 27 values of
      the column's own location, as before, and the columns run on "open or closed" rows that were bounds-checked, as before.)

The twin is oracle/lmconv_oracle.pixelcnn_forward in float64 on the host (state dict, one-hot input, masks cast to float64), once per
input (lru_cache) and never written to.  BAR = 1e-4 absolute on logits, the figure test_lmconv_gpu.py states for full-network logits.
err32 is the error of the SAME twin in fp32 on the host against that fp64 result: were it within a factor of three of BAR for an input
(> 3.3e-5), the input's seed would have to change -- checked on the CPU for every input below (test_the_fp32_twin_is_far_inside_the_bar
runs without a GPU call of the engine; largest err32 see MEASURED_MAXIMA).

"Fractional" = on masks made by c_oracle.unfolded_masks from real orders: a third of the open taps of the chosen locations scaled into
[0.25, 0.75], six of them set to 2.0 and six to -0.5, closed taps closed; frame 1 of the three distinct frames stays 0 / 1; every case
asserts that more than 20 % of the open taps it means to scale are not 1.

Orders: a random permutation of the locations outside two lattices of spacing 3, then the lattices (offsets differ per frame).  No two
locations of a lattice are tap neighbours (the taps reach 2), so a frame's walk is two wavefronts of 121 columns (32 x 32) / 12 (8 x 12),
and a batch of F frames launches 121 F columns at once: run_columns_tp takes k_column_tp8 up to 768 columns and k_column_tp beyond,
i.e. from 7 frames on (847 columns = 52 tiles of 16 + 15); 3 frames give 363 = 45 tiles of 8 + 3.

Measured on the MI355X (printed by the tests): MEASURED_MAXIMA below."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle, lmconv_oracle as lo
from pixelsynth_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-4
NET_SEED = 5
GRIDS = [(32, 32), (8, 12)]
GEMM_DEFAULTS = dict(gemm_merge_min=8192, gemm_wg_min=256, gemm_ws_min=1024, item_sort=2, gemm_ws=7)
BIG = 1 << 30
MEASURED_MAXIMA = """
max |logit - fp64 twin| over the compared locations, and err32 of the fp32 twin on the host for the same input and frame, against
BAR = 1e-4 (logits of magnitude up to 3.2).  Every form of a case gives the same figures: the forms are bit-equal.
  (a) 32 x 32, every form   frame 0 (fractional) 1.48e-6, err32 1.56e-6      frame 1 (0 / 1) 1.24e-6, err32 1.47e-6
  (a)  8 x 12, every form   frame 0 (fractional) 1.30e-6, err32 1.49e-6      frame 1 (0 / 1) 1.05e-6, err32 1.24e-6
  (b) 32 x 32 prefix        frames 0 / 1 / 2: 1.17e-6 / 1.12e-6 / 1.14e-6, err32 1.76e-6 / 1.47e-6 / 1.58e-6 (walk, latency, tp8, tp)
  (b) 32 x 32 prefix+A      frames 0 / 1 / 2: 1.20e-6 / 1.12e-6 / 1.24e-6, err32 1.64e-6 / 1.47e-6 / 1.67e-6 (walk, latency, tp8, tp)
  (b)  8 x 12 prefix        frames 0 / 1 / 2: 9.1e-7 / 9.5e-7 / 9.6e-7,    err32 1.22e-6 / 1.24e-6 / 1.33e-6 (walk, latency)
  (b)  8 x 12 prefix+A      frames 0 / 1 / 2: 1.03e-6 / 9.5e-7 / 1.01e-6,  err32 1.27e-6 / 1.24e-6 / 1.35e-6 (tp8)
err32 over whole grids, the largest per input (test_the_fp32_twin_is_far_inside_the_bar): 2.3e-6 at 32 x 32, 1.7e-6 at 8 x 12.
Column launches per case (eng.launch_counts() differences: k_column / k_column_la / k_column_tp / k_column_tp8):
  32 x 32  walk, 3 frames      242 / 0 / 0 / 0        8 x 12  walk, 3 frames      24 / 0 / 0 / 0
  32 x 32  latency, 3 frames   0 / 6 / 0 / 0          8 x 12  latency, 5 frames   0 / 2 / 0 / 0
  32 x 32  tp8, 3 frames       0 / 0 / 0 / 2          8 x 12  tp8, 5 frames       0 / 0 / 0 / 2
  32 x 32  tp, 7 frames        0 / 0 / 2 / 0
(c) against the library BEFORE k_ctx_build's check, max |column logit - whole-grid logit| at the walked locations, status clean in
every case: walk and latency form 0 for a neighbour tap of 0.5 (their neighbour role multiplies), throughput form 0.214 (undilated) /
0.285 (dilated); the centre at 0.5: 0.248 (undilated) / 0.295 (dilated) and a dilated centre of 0: 0.631, in all three forms.
"""


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def make_net():
    """The network of test_lmconv_gpu.make_net."""
    from pixelsynth_amd.lmconv.layers import PONO
    from pixelsynth_amd.lmconv.model import OurPixelCNN
    net = OurPixelCNN(nr_resnet=2, nr_filters=80, input_channels=512, nr_logistic_mix=10, kernel_size=(3, 3), max_dilation=2,
                      weight_norm=False, feature_norm_op=lambda _c: PONO(), dropout_prob=0, conv_bias=True, conv_mask_weight=False,
                      rematerialize=False, binarize=False).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(NET_SEED).items()}, strict=True)
    return net.to(DEV)


# ---- inputs: three distinct frames per grid, all on the host ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(H, W):
    """-> dict: order_loc (3, L) int32, first, walked (3, L) bool by location, codes (3, L) int32 (the completed grids), masks (three
    (3, 9, L) f32 arrays of 0 / 1 values: type A, type B, type B dilated).  Both lattices of every frame have the same size."""
    L = H * W
    n_r, n_c = len(range(1, H, 3)), len(range(1, W, 3))   # (the lattice of offset 1 is the shorter one: all are cut to its size)
    offs = [((0, 0), (1, 1)), ((0, 1), (1, 0)), ((1, 1), (0, 0))]
    rs = np.random.RandomState(H * 1000 + W)
    order_loc, walked = [], np.zeros((3, L), bool)
    for b, (o1, o2) in enumerate(offs):
        lat = [[(dr + 3 * i) * W + dc + 3 * j for i in range(n_r) for j in range(n_c)] for dr, dc in (o1, o2)]
        last = set(lat[0] + lat[1])
        assert len(last) == 2 * n_r * n_c
        rest = np.array([q for q in range(L) if q not in last])
        order_loc.append(np.concatenate([rs.permutation(rest), lat[0], lat[1]]))
        walked[b, lat[0] + lat[1]] = True
    order_loc = np.stack(order_loc).astype(np.int32)
    first = L - 2 * n_r * n_c
    masks = [np.concatenate([c_oracle.unfolded_masks(np.stack(np.divmod(o, W), 1), H, W, 3, dil, typ) for o in order_loc])
             for dil, typ in ((1, "A"), (1, "B"), (2, "B"))]
    for m in masks:
        assert np.isin(m, (0.0, 1.0)).all()
    assert (masks[1][:, 4] == 1).all() and (masks[2][:, 4] == 1).all() and (masks[0][:, 4] == 0).all()
    codes = rs.randint(0, 512, size=(3, L)).astype(np.int32)
    return dict(order_loc=order_loc, first=first, walked=walked, codes=codes, masks=masks, per_wave=n_r * n_c)


def fractionalise(m, where, rs):
    """m (9, L) one frame's mask, scaled in place at the locations `where` (L,) bool -> the share of those locations' open taps that
    are no longer 1."""
    open_ = (m != 0) & where[None]
    pick = open_ & (rs.rand(*m.shape) < 1.0 / 3)
    m[pick] *= (0.25 + 0.5 * rs.rand(int(pick.sum()))).astype(np.float32)
    idx = np.argwhere(open_)
    few = idx[rs.choice(len(idx), 12, replace=False)]
    m[few[:6, 0], few[:6, 1]] = 2.0
    m[few[6:, 0], few[6:, 1]] = -0.5
    return float((m[open_] != 1.0).mean())


@functools.lru_cache(maxsize=None)
def masks_of(H, W, variant):
    """The three masks of the grid's frames under `variant` (frame 1 always stays 0 / 1):
    all       fractional values everywhere, in all three masks;
    prefix    fractional values, in all three masks, at the locations in front of `first` in the frame's order;
    prefix+A  prefix, and fractional type-A values at the walked locations as well."""
    fr = frames(H, W)
    masks = [m.copy() for m in fr["masks"]]
    rs = np.random.RandomState({"all": 11, "prefix": 12, "prefix+A": 13}[variant] + H)
    shares = []
    for b in (0, 2):
        for k in range(3):
            where = np.ones(H * W, bool) if variant == "all" else ~fr["walked"][b]
            shares.append(fractionalise(masks[k][b], where, rs))
        if variant == "prefix+A":
            shares.append(fractionalise(masks[0][b], fr["walked"][b], rs))
        if variant != "all":   # the walked locations' type-B values are untouched
            assert np.array_equal(masks[1][b][:, fr["walked"][b]], fr["masks"][1][b][:, fr["walked"][b]])
            assert np.array_equal(masks[2][b][:, fr["walked"][b]], fr["masks"][2][b][:, fr["walked"][b]])
    assert min(shares) > 0.2, shares            # the case cannot silently become a 0 / 1 case
    for k in range(3):
        assert np.array_equal(masks[k][1], fr["masks"][k][1]) and np.array_equal(masks[k] == 0, fr["masks"][k] == 0)
    return masks


@functools.lru_cache(maxsize=None)
def twin(H, W, variant):
    """-> (ref (3, 512, L) float64 of the completed grids under masks_of(variant), err32 (3,) of the fp32 twin against it)."""
    fr, masks = frames(H, W), masks_of(H, W, variant)
    sd = {k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(NET_SEED).items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    x = torch.nn.functional.one_hot(torch.from_numpy(fr["codes"].astype(np.int64)).view(3, H, W), 512).permute(0, 3, 1, 2)
    with torch.no_grad():
        ref = lo.pixelcnn_forward(sd64, x.double(), *[torch.from_numpy(m).double() for m in masks]).reshape(3, 512, H * W).numpy()
        r32 = lo.pixelcnn_forward(sd, x.float(), *[torch.from_numpy(m) for m in masks]).reshape(3, 512, H * W).numpy()
    assert np.isfinite(ref).all()
    ref.setflags(write=False)
    return ref, np.abs(r32 - ref).max(axis=(1, 2))


INPUTS = [(H, W, v) for H, W in GRIDS for v in ("all", "prefix", "prefix+A")]


@pytest.mark.parametrize("H,W,variant", INPUTS)
def test_the_fp32_twin_is_far_inside_the_bar(H, W, variant):
    """err32 of every input this file uses stays a factor of three inside BAR, so BAR measures the engine and not the input (host only)."""
    err32 = twin(H, W, variant)[1]
    print(f"err32 {H}x{W} {variant}: " + " ".join(f"{e:.2e}" for e in err32))
    assert err32.max() * 3 < BAR


def _report(tag, got, ref, err32):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"MEASURED {tag}: max err {err:.3e}  err32 {float(err32):.3e}")
    return err


# ---- (a) the whole-grid forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", GRIDS)
def test_whole_grid_forms_with_fractional_masks_against_the_fp64_twin(H, W):
    fr, masks = frames(H, W), masks_of(H, W, "all")
    ref, err32 = twin(H, W, "all")
    eng = make_net().engine(H, W, 2)
    codes, ms = tt(fr["codes"][:2]), [tt(m[:2]) for m in masks]   # frame 0 fractional (type A included), frame 1 0 / 1
    run = lambda: eng.forward(codes, *ms).reshape(2, 512, H * W).cpu()
    forms = [("k_gemm", dict(gemm_merge_min=0, gemm_wg_min=BIG), ("k_gemm",)),
             ("k_gemm_wg", dict(gemm_wg_min=1, gemm_ws=0, gemm_ws_min=1), ("k_gemm_wg",)),
             ("k_gemm_ws", dict(gemm_ws=7), ("k_gemm_ws<0>", "k_gemm_ws<1>", "k_gemm_ws<2>")),
             ("gemm_ws=2", dict(gemm_ws=2), ("k_gemm_ws<1>", "k_gemm_wg")),
             ("item_sort=0", dict(gemm_ws=0, item_sort=0), ("k_gemm_wg",))]
    out = {}
    try:
        for name, cfg, kinds in forms:
            eng.set_tuning(**cfg)
            n0 = eng.launch_counts()
            out[name] = run()
            n1 = eng.launch_counts()
            for k in kinds:
                assert n1[k] > n0[k], (name, k)                  # the form under test is the one that ran
            if name == "k_gemm":
                assert all(n1[k] == n0[k] for k in n1 if k != "k_gemm"), name
    finally:
        eng.set_tuning(**GEMM_DEFAULTS)
    for name in out:
        assert torch.equal(out[name], out["k_gemm"]), name
        for b in range(2):
            assert _report(f"(a) {H}x{W} {name} frame {b}", out[name][b].numpy(), ref[b], err32[b]) <= BAR, (name, b)
    eng.check()


# ---- (b) AR runs over a prefix computed under fractional masks --------------------------------------------------------------------
def _ar_inputs(H, W, F_, masks):
    from pixelsynth_amd.lmconv.model import wavefronts
    fr = frames(H, W)
    idx = np.arange(F_) % 3
    order_loc = fr["order_loc"][idx]
    reg = fr["walked"][idx].astype(np.uint8)
    final = fr["codes"][idx]
    start = final.copy()
    start[reg == 1] = (start[reg == 1] + 7) % 512        # what stands at the sampled locations beforehand must not matter
    waves = wavefronts(order_loc, H, W, fr["first"], DEV, max_cols=1024)
    assert np.array_equal(np.diff(waves[1]), [F_ * fr["per_wave"]] * 2)
    return dict(idx=idx, order=tt(order_loc), reg=tt(reg), reg_host=reg, final=final, start=start, waves=waves, first=fr["first"],
                ms=[tt(m[idx]) for m in masks])


def _run_form(eng, form, a, forced=None, uniforms=None):
    """One AR run in `form` -> (codes, logits or None, launch-count differences)."""
    tp_default = eng.get_tuning("tp_min_cols")
    c = tt(a["start"].copy())
    kw = dict(temperature=0.7, forced=forced, uniforms=uniforms, first_step=a["first"])
    n0 = eng.launch_counts()
    try:
        if form in ("latency", "tp8", "tp"):
            eng.set_tuning(tp_min_cols=BIG if form == "latency" else 1)
        if form == "prefix_columns":
            eng.ar_prefix(c, a["order"], a["reg"], *a["ms"], a["first"])
            eng.ar_columns(c, a["order"], a["reg"], *a["ms"], a["waves"], **kw)
            out = None
        else:
            out = eng.ar_run(c, a["order"], a["reg"], *a["ms"], want_logits=True, waves=None if form == "walk" else a["waves"], **kw)
        torch.cuda.synchronize()
    finally:
        eng.set_tuning(tp_min_cols=tp_default)
    n1 = eng.launch_counts()
    return c, out, {k: n1[k] - n0[k] for k in n1 if k.startswith("k_column")}


def _expect_kernels(form, d):
    lat, tp16, tp8 = d["k_column"] + d["k_column_la"], d["k_column_tp"], d["k_column_tp8"]
    if form == "walk":
        assert d["k_column"] > 0 and d["k_column_la"] == 0 and tp16 == 0 and tp8 == 0, d
    elif form == "latency":
        assert lat > 0 and tp16 == 0 and tp8 == 0, d
    elif form in ("tp8", "prefix_columns"):   # (the split calls at the default tuning: 363 columns a wave are throughput-form launches)
        assert tp8 > 0 and lat == 0 and tp16 == 0, d
    else:
        assert tp16 > 0 and lat == 0 and tp8 == 0, d


# launch counts seen on the MI355X: see MEASURED_MAXIMA
B_CASES = [(32, 32, "walk", 3, "prefix"), (32, 32, "latency", 3, "prefix"), (32, 32, "tp8", 3, "prefix"), (32, 32, "tp", 7, "prefix"),
           (32, 32, "prefix_columns", 3, "prefix"),
           (32, 32, "walk", 3, "prefix+A"), (32, 32, "latency", 3, "prefix+A"), (32, 32, "tp8", 3, "prefix+A"), (32, 32, "tp", 7, "prefix+A"),
           (8, 12, "walk", 3, "prefix"), (8, 12, "latency", 5, "prefix"), (8, 12, "tp8", 5, "prefix+A")]


@pytest.mark.parametrize("H,W,form,F_,variant", B_CASES)
def test_columns_over_a_fractional_prefix_are_the_whole_grid_pass(H, W, form, F_, variant):
    """(b).  Teacher-forced; the split prefix / columns calls return no logits, so there the codes DRAWN from given uniforms must be
    those of ar_run with the same uniforms, whose logits are held to both checks."""
    masks = masks_of(H, W, variant)
    ref, err32 = twin(H, W, variant)
    a = _ar_inputs(H, W, F_, masks)
    eng = make_net().engine(H, W, F_)
    L = H * W
    if form == "prefix_columns":
        u = tt(np.random.RandomState(F_).rand(F_, L).astype(np.float32))
        c_split, _, d = _run_form(eng, form, a, uniforms=u)
        eng.check()
        _expect_kernels(form, d)
        c, out, _ = _run_form(eng, "latency", a, uniforms=u)
        eng.check()
        assert torch.equal(c_split, c)
        final = c.cpu().numpy()
        assert (final[a["reg_host"] == 1] != a["start"][a["reg_host"] == 1]).any()
    else:
        c, out, d = _run_form(eng, form, a, forced=tt(a["final"]))
        eng.check()
        print(f"MEASURED (b) {H}x{W} {form} {F_} frames {variant}: launches {d}")
        _expect_kernels(form, d)
        final = a["final"]
        assert np.array_equal(c.cpu().numpy(), final)
    full = eng.forward(tt(final), *a["ms"]).reshape(F_, 512, L).permute(0, 2, 1)
    eng.check()
    sel = a["reg"].bool()
    assert torch.equal(out[sel], full[sel])                      # a column is the whole-grid pass's value at its location
    assert torch.isfinite(out[sel]).all()
    got = out.cpu().numpy()
    if form != "prefix_columns":                                 # (drawn codes are not the twin's input)
        for b in range(F_):
            w = a["reg_host"][b] == 1
            tag = f"(b) {H}x{W} {form} {F_} frames {variant} frame {b}"
            assert _report(tag, got[b][w], ref[b % 3][:, w].T, err32[b % 3]) <= BAR, tag
            if b >= 3:
                assert np.array_equal(got[b][w], got[b - 3][w])  # copies of a frame agree wherever they sit in a tile


# ---- (c) an offending value at a walked location ----------------------------------------------------------------------------------
C_VALUES = {"undilated_neighbour_0.5": (1, "nbr", 0.5), "dilated_neighbour_0.5": (2, "nbr", 0.5), "undilated_centre_0.5": (1, "centre", 0.5),
            "dilated_centre_0.5": (2, "centre", 0.5), "undilated_neighbour_nan": (1, "nbr", float("nan")),
            "dilated_centre_0": (2, "centre", 0.0)}       # (a closed centre is 0 / 1 -- and still not what the chain role computes)
C_FORMS = ["walk", "latency", "tp8"]
C_F = 3


def offending_masks(case):
    """The 0 / 1 masks of the 32 x 32 frames with ONE value replaced, at a walked location in the middle of frame 0's first lattice
    -> (masks, frame, location)."""
    kind, where, value = C_VALUES[case]
    fr = frames(32, 32)
    masks = [m.copy() for m in fr["masks"]]
    q = 15 * 32 + 15
    assert fr["walked"][0, q] and np.nonzero(fr["order_loc"][0] == q)[0][0] >= fr["first"]
    tap = 4 if where == "centre" else int(np.nonzero(masks[kind][0][:, q] * (np.arange(9) != 4))[0][0])
    assert masks[kind][0][tap, q] == 1.0
    masks[kind][0][tap, q] = value
    return masks, 0, q


@functools.lru_cache(maxsize=None)
def _fresh_handle_bits(form):
    """The 0 / 1 run of the 32 x 32 frames on a handle that has seen nothing else -> (codes, logits) on the host."""
    from pixelsynth_amd.lmconv.model import PixelCNNEngine
    a = _ar_inputs(32, 32, C_F, frames(32, 32)["masks"])
    eng = PixelCNNEngine(make_net().state_dict(), 32, 32, C_F)
    try:
        c, out, _ = _run_form(eng, form, a, uniforms=tt(np.random.RandomState(3).rand(C_F, 1024).astype(np.float32)))
        eng.check()
        return c.cpu(), out.cpu()
    finally:
        eng.close()


def run_offending(eng, form, case):
    """-> (logits of the run, whole-grid logits on the completed grid under the same masks, walked selector, the text
    ps_pixelcnn_status raised or None)."""
    masks, _, _ = offending_masks(case)
    a = _ar_inputs(32, 32, C_F, masks)
    c, out, d = _run_form(eng, form, a, forced=tt(a["final"]))
    try:
        eng.check()
        raised = None
    except RuntimeError as e:
        raised = str(e)
    _expect_kernels(form, d)
    full = eng.forward(tt(a["final"]), *a["ms"]).reshape(C_F, 512, 1024).permute(0, 2, 1)
    return out, full, a["reg"].bool(), raised


@pytest.mark.parametrize("case", list(C_VALUES))
@pytest.mark.parametrize("form", C_FORMS)
def test_an_offending_type_b_value_at_a_walked_location_is_refused(form, case):
    eng = make_net().engine(32, 32, C_F, slot=40)
    eng.check()
    _, _, _, raised = run_offending(eng, form, case)
    assert raised is not None and "mask values" in raised, raised
    assert "wait ran out" not in raised and "outside this run" not in raised, raised
    eng.check()                                                  # reported once
    # ... and the handle stays usable: the 0 / 1 masks on it give the bits of a fresh handle
    a = _ar_inputs(32, 32, C_F, frames(32, 32)["masks"])
    c, out, _ = _run_form(eng, form, a, uniforms=tt(np.random.RandomState(3).rand(C_F, 1024).astype(np.float32)))
    eng.check()
    c0, out0 = _fresh_handle_bits(form)
    sel = a["reg"].bool().cpu()
    assert torch.equal(c.cpu(), c0)
    assert torch.equal(out.cpu()[sel], out0[sel]) and torch.isfinite(out0[sel]).all()
    assert (c0.numpy()[a["reg_host"] == 1] != a["start"][a["reg_host"] == 1]).any()


def test_the_prefix_pass_and_the_forward_keep_any_value():
    """The refusal is the columns' alone.  An AR run whose walked locations are 0 / 1 stays clean whatever its prefix holds: (b) asserts
    that.  Here: the whole-grid forward of masks that an AR run would refuse leaves the status clean."""
    masks, _, _ = offending_masks("undilated_centre_0.5")
    fr = frames(32, 32)
    eng = make_net().engine(32, 32, C_F, slot=40)
    out = eng.forward(tt(fr["codes"]), *[tt(m) for m in masks])
    eng.check()
    assert torch.isfinite(out).all()
