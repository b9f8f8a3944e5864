"""The fp64 definition of what ps_code_nll_f32 (include/pixelsynth_nll.h) computes, in numpy: per location the negative log-likelihood
of the target code under softmax(logits / T), the entropy of that distribution and whether the target is the arg-max; per frame the
sums over the observed (0) and the sampled (1) locations.  tests/test_code_nll_cpu.py pins it to torch.nn.functional.cross_entropy and
to closed forms; the GPU tests pin the kernel to it."""
import numpy as np

CLASSES = 512


def code_nll_ref64(logits, targets, region=None, temperature=1.0, layout="chw"):
    """logits (F,C,L) for layout "chw" or (F,L,C) for "lc", any float type (taken to fp64 as they are); targets (F,L) int; region (F,L),
    nonzero = sampled, or None: all observed -> dict(nll (F,L) f64, entropy (F,L) f64, hit (F,L) uint8, frames (F,2,4) f64:
    [f][g] = count, sum nll, sum entropy, sum hit of group g).  A NaN logit gives a NaN nll at its location; a target outside
    [0, C) gives a NaN nll and hit 0; an empty group gives zeros."""
    x = np.asarray(logits, np.float64)
    if layout == "chw":
        x = np.swapaxes(x, 1, 2)
    elif layout != "lc":
        raise ValueError(f"layout {layout!r}")
    x = np.ascontiguousarray(x) / float(temperature)         # (F,L,C), one memory order: the sums are the same bits for both layouts
    F_, L, C = x.shape
    t = np.asarray(targets).reshape(F_, L).astype(np.int64)
    valid = (t >= 0) & (t < C)
    tc = np.where(valid, t, 0)
    finite = np.where(np.isnan(x), -np.inf, x)
    m = finite.max(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = x - m
        e = np.exp(d)
        s = e.sum(-1)
        lse = np.log(s)
        nll = lse - np.take_along_axis(d, tc[..., None], -1)[..., 0]
        nll = np.where(valid, nll, np.nan)
        p_logp = np.where(e > 0, e * d, np.where(np.isnan(e), np.nan, 0.0))   # a class whose exp is 0 contributes 0, never 0 * -inf
        entropy = lse - p_logp.sum(-1) / s
    hit = (valid & (finite.argmax(-1) == t)).astype(np.uint8)                 # argmax: the first (lowest) class among equal maxima
    g = np.zeros((F_, L), bool) if region is None else np.asarray(region).reshape(F_, L) != 0
    frames = np.zeros((F_, 2, 4), np.float64)
    for f in range(F_):
        for k, sel in enumerate((~g[f], g[f])):
            frames[f, k] = [sel.sum(), nll[f][sel].sum(), entropy[f][sel].sum(), hit[f][sel].sum()]
    return dict(nll=nll, entropy=entropy, hit=hit, frames=frames)


def rounding_bound(logits, temperature=1.0, layout="chw"):
    """(F,L) f64: 2^-23 (2 a + 32) with a = max |x / T| over the classes of a location (NaN logits left out): the rounding bound of the
    fp32 computation of the nll (tests/test_code_nll_gpu.py states the derivation); the entropy's is this times ln C."""
    x = np.abs(np.asarray(logits, np.float64)) / float(temperature)
    a = np.nanmax(x, axis=1 if layout == "chw" else 2)
    return 2.0 ** -23 * (2.0 * a + 32.0)
