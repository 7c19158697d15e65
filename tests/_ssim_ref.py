"""The float64 restatement the reconstruction-fidelity tests hold the device to (ggan_ssim_pairs, functional.ssim_pairs / psnr_from_mse,
Evaluator.rec_scores, SequenceEvaluator.rec_scores): per-image mean squared error and mean structural similarity (Wang, Bovik, Sheikh,
Simoncelli 2004) with the DIRECT 2-D window -- the outer product of the 11 taps over every valid position, deliberately not the separable
trick the kernel uses --, built from the fp32 inputs with the unit-scale maps in float64; plus the cached, read-only recipes of the cases
that tests/test_rec_cpu.py and tests/test_rec_gpu.py share.

The filter, crop and constants are those of scikit-image's structural_similarity(gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=1): an 11-tap Gaussian (truncate 3.5) normalised to sum 1, the map cropped by 5 on every side,
population variances and covariance, C1 = 0.01^2, C2 = 0.03^2.

The gate is the project's one for set-level values (_parzen_ref.gate): |got - ref| <= 2e-5 max(1, |ref|), per image."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

GATE = 2e-5
C1, C2 = 0.01 ** 2, 0.03 ** 2
TAPS, SIGMA = 11, 1.5
SHAPES = [(1, 1, 11, 11), (5, 1, 12, 17), (67, 1, 28, 28), (33, 3, 32, 32), (9, 1, 64, 64), (6, 3, 64, 64)]
# beyond the list every kind runs at: a plane size that is no multiple of 4 floats (every second plane starts off a 16-byte boundary: both
# load paths in one call), and a plane of two bands with a ragged second one whose width differs from its height
EXTRA_SHAPES = [(7, 2, 13, 17), (3, 1, 64, 37), (4, 4, 40, 64)]
KINDS = ['smooth', 'smooth_fine', 'binary_dimmed', 'noise', 'bright_flat', 'two_maps']
TANH, SIGMOID, BYTES = (0.5, 0.5), (1.0, 0.0), (1.0 / 255.0, 0.0)


def gate(ref):
    return GATE * np.maximum(1.0, np.abs(ref))


def taps():
    """the 11 taps of the window in float64: exp(-k^2 / (2 sigma^2)), k = -5 .. 5, normalised to sum 1"""
    k = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    g = np.exp(-0.5 * k * k / (SIGMA * SIGMA))
    return g / g.sum()


def window():
    """the 2-D window [11, 11]: the outer product of the taps (sums to 1)"""
    g = taps()
    return np.outer(g, g)


def unit(x, m):
    """fp32 values as handed to the kernel -> unit-scale pixels in float64"""
    return float(m[0]) * np.asarray(x, np.float64) + float(m[1])


def ssim_map(ua, ub):
    """the SSIM map [..., h - 10, w - 10] of unit-scale planes [..., h, w] in float64, by the direct 2-D window"""
    W = window()
    pa, pb = sliding_window_view(ua, (TAPS, TAPS), axis=(-2, -1)), sliding_window_view(ub, (TAPS, TAPS), axis=(-2, -1))
    mx, my = np.einsum('...ij,ij->...', pa, W), np.einsum('...ij,ij->...', pb, W)
    # population moments about the window means (the definition; no E[x^2] - mx^2 in the reference)
    da, db = pa - mx[..., None, None], pb - my[..., None, None]
    sxx, syy, sxy = (np.einsum('...ij,...ij,ij->...', p, q, W) for p, q in ((da, da), (db, db), (da, db)))
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def pairs(a, b, shape, map_a=SIGMOID, map_b=None):
    """(mse [n], ssim [n]) in float64 of rows a[i] against b[i], rows [n, c*h*w] of channel-major planes"""
    c, h, w = shape
    map_b = map_a if map_b is None else map_b
    ua = unit(a, map_a).reshape(-1, c, h, w)
    ub = unit(b, map_b).reshape(-1, c, h, w)
    mse = ((ua - ub) ** 2).mean(axis=(1, 2, 3))
    ssim = np.stack([ssim_map(ua[i], ub[i]).mean() for i in range(ua.shape[0])])       # (an image at a time: the windows of one fit in cache)
    return mse, ssim


def psnr(mse):
    """-10 log10(max(mse, 1e-10)) in float64: a perfect image scores 100 dB"""
    return -10.0 * np.log10(np.maximum(np.asarray(mse, np.float64), 1e-10))


def pass_values(mse, ssim):
    """the four logged values from per-image rows, in float64: mean mse, mean per-image psnr, mean ssim, its standard error (the population
    std / sqrt(count), as the Parzen pass)"""
    mse, ssim = np.asarray(mse, np.float64), np.asarray(ssim, np.float64)
    return {'dev rec mse x': mse.mean(), 'dev rec psnr x': psnr(mse).mean(), 'dev rec ssim x': ssim.mean(),
            'dev rec ssim se x': ssim.std() / np.sqrt(len(ssim))}


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------------
def _smooth(rng, n, c, h, w):
    """image-like planes in [0.1, 0.9]: a few low-frequency waves per plane"""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
    out = np.zeros((n, c, h, w))
    for _ in range(3):
        f = rng.uniform(0.5, 4.0, size=(n, c, 2, 1, 1))
        p = rng.uniform(0, 2 * np.pi, size=(n, c, 1, 1))
        out += np.sin(2 * np.pi * (f[:, :, 0] * yy + f[:, :, 1] * xx) + p)
    return 0.5 + 0.4 * out / 3.0


@functools.lru_cache(maxsize=None)
def case(kind, n, c, h, w):
    """(a, b, map_a, map_b): read-only fp32 rows [n, c*h*w] as the kernel is handed them, and their unit-scale maps"""
    rng = np.random.default_rng([KINDS.index(kind), n, c, h, w])
    ma = mb = SIGMOID
    if kind in ('smooth', 'smooth_fine'):
        a = _smooth(rng, n, c, h, w)
        b = a + (0.05 if kind == 'smooth' else 1e-3) * rng.standard_normal(a.shape)
    elif kind == 'binary_dimmed':                    # binary MNIST-like strokes against a dimmed copy
        a = (_smooth(rng, n, c, h, w) > 0.6).astype(np.float64)
        b = 0.7 * a
    elif kind == 'noise':                            # uncorrelated: SSIM near 0, some values negative
        a, b = rng.random((n, c, h, w)), rng.random((n, c, h, w))
    elif kind == 'bright_flat':                      # where E[x^2] - mx^2 cancels in fp32 and C2 is all that stands in the denominator
        a = 0.98 + 1e-3 * rng.standard_normal((n, c, h, w))
        b = 0.98 + 1e-3 * rng.standard_normal((n, c, h, w))
    elif kind == 'two_maps':                         # tanh range against data in 0..255
        u = _smooth(rng, n, c, h, w)
        a = 2.0 * (u + 0.05 * rng.standard_normal(u.shape)) - 1.0
        b = np.round(255.0 * u)
        ma, mb = TANH, BYTES
    else:
        raise ValueError(kind)
    a, b = (np.ascontiguousarray(v.reshape(n, c * h * w), dtype=np.float32) for v in (a, b))
    a.flags.writeable = b.flags.writeable = False
    return a, b, ma, mb


@functools.lru_cache(maxsize=None)
def reference(kind, n, c, h, w):
    a, b, ma, mb = case(kind, n, c, h, w)
    mse, ssim = pairs(a, b, (c, h, w), ma, mb)
    mse.flags.writeable = ssim.flags.writeable = False
    return mse, ssim


# ---- the kernel's formulation in float32, for the CPU tests: what the centring buys ------------------------------------------------------
def pairs_f32(a, b, shape, map_a=SIGMOID, map_b=None, centred=True):
    """ssim [n] by separable one-pass moments in float32 -- centred by each plane's mean as the kernel, or raw -- (numpy float32 arithmetic,
    not the kernel's order: the size of the cancellation is what this shows)"""
    c, h, w = shape
    map_b = map_a if map_b is None else map_b
    f = np.float32
    g = taps().astype(f)
    ua = (f(map_a[0]) * np.asarray(a, f) + f(map_a[1])).reshape(-1, c, h, w)
    ub = (f(map_b[0]) * np.asarray(b, f) + f(map_b[1])).reshape(-1, c, h, w)
    ca = ua.mean(axis=(2, 3), keepdims=True, dtype=f) if centred else f(0)
    cb = ub.mean(axis=(2, 3), keepdims=True, dtype=f) if centred else f(0)
    x, y = ua - ca, ub - cb

    def blur(v):
        rows = sum(g[k] * v[..., :, k:k + w - 10] for k in range(TAPS))
        return sum(g[k] * rows[..., k:k + h - 10, :] for k in range(TAPS))
    dx, dy, exx, eyy, exy = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    mx, my = ca + dx, cb + dy
    sxx, syy, sxy = exx - dx * dx, eyy - dy * dy, exy - dx * dy
    m = ((f(2) * mx * my + f(C1)) * (f(2) * sxy + f(C2))) / ((mx * mx + my * my + f(C1)) * (sxx + syy + f(C2)))
    assert m.dtype == f
    return m.astype(np.float64).mean(axis=(1, 2, 3))
