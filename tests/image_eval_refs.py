"""Camera image evaluation (csrc/image_eval.hip): restatements of torchmetrics' PSNR / SSIM, the test images, an fp32
emulation of the kernel's accumulation order and the per-window error bound ``B``.  Used by tests/test_image_eval_host.py,
tests/test_gpu_image_eval.py, tests/test_image_eval_plugin_host.py and scripts/bench_image_eval.py.

Why restatements: torchmetrics is installed on none of the machines (oracle/ref_import.py stubs it), so the definition is the
specification: ``structural_similarity_index_measure(preds, target)`` with its defaults (11 x 11 Gaussian window, sigma 1.5,
k1 0.01, k2 0.03, data_range None = max over both images of max - min, reflect pad, crop of the padded border, mean) and
``PeakSignalNoiseRatio(data_range=1.0)``.  ``ssim_padded`` is written the way torchmetrics does it, in float64 or fp32, with
and without the variance clamp of its newer versions; ``ssim_valid`` is the same thing over the windows that lie inside the
image, in float64, and is THE reference of the tests.

The kernel (per tile of T x T windows and per channel; u = 2^-24, g_i the fp32 taps, every operation rounded once, the
library builds with -ffp-contract=off and writes its fmaf explicitly):

    a' = fl(a - p), b' = fl(b - q)                      p, q: the pixel 21 rows / columns into the tile's halo, clamped
    h  = fma(g_10, v_10, ... fma(g_1, v_1, fl(g_0 v_0)))    along the row, for v = a', b', fl(a'a'), fl(b'b'), fl(a'b')
    m  = the same chain down the column of h                -> ma, mb, maa, mbb, mab
    va = fl(maa - fl(ma ma)), vb likewise, cov = fl(mab - fl(ma mb)), mua = fl(p + ma), mub = fl(q + mb)
    s  = fl(fl(fl(2 fl(mua mub) + c1) fl(2 cov + c2)) / fl(fl(fl(fl(mua mua) + fl(mub mub)) + c1) fl(fl(va + vb) + c2)))

Per-moment bounds.  A chain of 11 taps has 10 additions; the first product is rounded, the others are fused.  So the tap v_0
collects 11 roundings and every other at most 10: |h - sum g_i v_i| <= 11 u sum g_i |v_i| to first order, and the same again
for the column pass: 22 u.  That is (k + 2) u sum g |v| with k = 20, the number of additions in the two passes.  On top
of the accumulation come the roundings that happen before it: each tap is the float64 tap rounded to fp32 (1 u per pass:
2 u), the shift a' = fl(a - p) (1 u on a', hence 1 u on the linear moments and 2 u on the quadratic ones) and the product
fl(a'a') (1 u, quadratic moments only).  Altogether, with v the shifted values and g (x) g the exact window,

    |ma  - sum g a'|    <= (k + 5) u sum g |a'|     = K_LIN  u sum g |a'|       K_LIN  = 25
    |maa - sum g a'^2|  <= (k + 7) u sum g a'^2     = K_QUAD u sum g a'^2       K_QUAD = 27     (mbb, mab likewise)

The shift does not change va, vb, cov, and mua = p + ma, so these ARE bounds on the reference's own moments.  They are bounded
by the local contrast, not by the pixel value: that is what the shift buys.

Propagation (``window_bound``).  Every later operation z = x o y is one rounded fp32 operation: its absolute error is the
first-order propagation of its operands' errors plus u |z| (``_V`` below: a value with its error; doubling is exact).
c1 and c2 are formed in float64 from the exact range and rounded once: u c1, u c2.  The quotient is IEEE-rounded: u |s|.
B is the error of s that comes out.  Nothing in B is fitted to what the kernel gives.

Scalars.  ssim is the float64 sum of the fp32 s, divided by the count, rounded once: within 1 ulp of the float64 mean of the
kernel's own map, and within mean(B) + u of the float64 value.  psnr: the difference is one rounded fp32 subtraction (u), its
square and the sum are float64: mse within 2 u (1 + 2^-29) relative, which the issue's 4 u covers; 10 log10 turns a relative
error e into (10 / ln 10) e; the final rounding adds 1 ulp.
"""
import numpy as np
import torch

import synth

U = 2.0 ** -24
TAPS, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
TILE = 32            # NRHIP_SSIM_TILE
PIVOT = (TILE + TAPS - 1) // 2
ADDS = 2 * (TAPS - 1)  # k: additions of the two passes
K_LIN, K_QUAD = ADDS + 5, ADDS + 7
PSNR_REL = 4 * U     # relative bound on the mean squared error (the issue's figure)
KINDS = ("noise", "smooth", "flat", "dark")


def window(sigma=SIGMA, total=1.0):
    """float64 taps exp(-(d / sigma)^2 / 2), d = -5..5, normalised to ``total``"""
    d = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    g = np.exp(-((d / sigma) ** 2) / 2)
    return g / g.sum() * total


def data_range(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return max(a.max() - a.min(), b.max() - b.min())


def psnr(a, b, psnr_range=1.0):
    """float64; +inf for identical images"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.float64(psnr_range) ** 2 / np.mean((a - b) ** 2))


def psnr_bound(value):
    """|psnr - float64| allowed for an fp32 result near ``value``: (10 / ln 10) 4u + 1 ulp"""
    return 10.0 / np.log(10.0) * PSNR_REL + float(np.spacing(np.float32(abs(value))))


# ---- as torchmetrics does it --------------------------------------------------------------------------------------------
def ssim_padded(a, b, dtype=torch.float64, clamp=False, return_map=False, pad=True):
    """[H,W,C] images -> ssim: reflect pad by 5, ONE grouped conv2d over the five stacked images, crop of the padded border,
    mean; every step in ``dtype``.  clamp: the variances clamped at 0, as newer torchmetrics versions do.  pad=False: the
    same arithmetic without the pad and without the crop -- the windows that lie inside the image."""
    p = torch.as_tensor(np.array(a)).to(dtype).permute(2, 0, 1)[None]
    t = torch.as_tensor(np.array(b)).to(dtype).permute(2, 0, 1)[None]
    c = p.shape[1]
    r = torch.maximum(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (K1 * r) ** 2, (K2 * r) ** 2
    n = (TAPS - 1) // 2
    g = torch.as_tensor(window()).to(dtype)
    kernel = (g[:, None] * g[None, :]).expand(c, 1, TAPS, TAPS).contiguous()
    if pad:
        p = torch.nn.functional.pad(p, (n, n, n, n), mode="reflect")
        t = torch.nn.functional.pad(t, (n, n, n, n), mode="reflect")
    out = torch.nn.functional.conv2d(torch.cat([p, t, p * p, t * t, p * t]), kernel, groups=c)
    mu_p, mu_t, e_pp, e_tt, e_pt = (out[i:i + 1] for i in range(5))
    mu_pp, mu_tt, mu_pt = mu_p * mu_p, mu_t * mu_t, mu_p * mu_t
    var_p, var_t, cov = e_pp - mu_pp, e_tt - mu_tt, e_pt - mu_pt
    if clamp:
        var_p, var_t = var_p.clamp(min=0.0), var_t.clamp(min=0.0)
    s = ((2 * mu_pt + c1) * (2 * cov + c2)) / ((mu_pp + mu_tt + c1) * (var_p + var_t + c2))
    if pad:
        s = s[..., n:-n, n:-n]
    m = s[0].permute(1, 2, 0).double().numpy()
    return (float(s.double().mean()), m) if return_map else float(s.double().mean())


def conv_form_float64_error(a, b):
    """what float64 itself loses in E[x^2] - mu^2 on the raw values: each second moment is a sum of 121 products of size up
    to max x^2, so it carries up to 122 * 2^-53 max x^2, twice that for the two variances, against a denominator of at least
    c2 -- first order, with the same again for everything else: 512 * 2^-53 max x^2 / c2"""
    x2 = max(float(np.max(np.asarray(a, np.float64) ** 2)), float(np.max(np.asarray(b, np.float64) ** 2)))
    return 512 * 2.0 ** -53 * x2 / (K2 * data_range(a, b)) ** 2 + 1e-14


# ---- the windows that lie inside the image, float64, from the definition -----------------------------------------------
def _blur(x, g):
    """valid separable 11-tap correlation of [H,W,...] along the first two axes"""
    v = np.lib.stride_tricks.sliding_window_view(x, TAPS, axis=1)
    x = np.tensordot(v, g, axes=([-1], [0]))
    v = np.lib.stride_tricks.sliding_window_view(x, TAPS, axis=0)
    return np.tensordot(v, g, axes=([-1], [0]))


def ssim_valid(a, b, g=None, k2=K2, r=None, shift=0):
    """float64 map [H-10, W-10, C] of s over every window inside the image, THE reference of the tests.  Two passes per
    window: the means, then the central moments sum w (x - mu)^2 -- no cancellation at all; the issue's sigma^2 = sum w x^2
    - mu^2 equals sum w (x - mu)^2 + mu^2 (1 - sum w), and that term is kept (it is 1e-16 for the true window and what makes
    a window that sums to 1.001 wrong).  The keyword arguments are for the WRONG restatements the host test needs: another
    window, another k2, another range, the window moved by ``shift`` pixels down and right (edge-replicated there)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = window() if g is None else g
    r = data_range(a, b) if r is None else r
    c1, c2 = (K1 * r) ** 2, (k2 * r) ** 2
    if shift:
        a, b = (np.pad(x, ((0, shift), (0, shift), (0, 0)), mode="edge")[shift:, shift:] for x in (a, b))
    w2 = g[:, None] * g[None, :]
    rest = 1.0 - w2.sum()
    wa = np.lib.stride_tricks.sliding_window_view(a, (TAPS, TAPS), axis=(0, 1))  # [H-10, W-10, C, 11, 11]
    wb = np.lib.stride_tricks.sliding_window_view(b, (TAPS, TAPS), axis=(0, 1))
    mu_a, mu_b = (wa * w2).sum((-2, -1)), (wb * w2).sum((-2, -1))
    da, db = wa - mu_a[..., None, None], wb - mu_b[..., None, None]
    var_a = (da * da * w2).sum((-2, -1)) + mu_a * mu_a * rest
    var_b = (db * db * w2).sum((-2, -1)) + mu_b * mu_b * rest
    cov = (da * db * w2).sum((-2, -1)) + mu_a * mu_b * rest
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))


def ssim_valid_padded(a, b):
    """the same two-pass arithmetic the way torchmetrics lays the windows out: reflect pad by 5, every window of the padded
    image, crop of the padded border"""
    n = (TAPS - 1) // 2
    pa, pb = (np.pad(np.asarray(x, np.float64), ((n, n), (n, n), (0, 0)), mode="reflect") for x in (a, b))
    return ssim_valid(pa, pb)[n:-n, n:-n]


# ---- the kernel's tiling ------------------------------------------------------------------------------------------------
def tiles(h, w, tile=TILE):
    """(y0, x0, py, px) of every tile: origin of its windows (= of its halo) and its pivot pixel"""
    for y0 in range(0, h - TAPS + 1, tile):
        for x0 in range(0, w - TAPS + 1, tile):
            yield y0, x0, min(y0 + PIVOT, h - 1), min(x0 + PIVOT, w - 1)


def _halo(img, y0, x0, pivot, tile):
    """the fp32 shifted halo [tile + 10, tile + 10, C] of a tile, zero outside the image"""
    n = tile + TAPS - 1
    out = np.zeros((n, n, img.shape[2]), np.float32)
    part = img[y0:y0 + n, x0:x0 + n]
    out[:part.shape[0], :part.shape[1]] = part - pivot  # fp32 - fp32: one rounding
    return out


def _fma(g, v, acc):
    """fp32 fma of fp32 operands: the product is exact in float64, the sum is rounded to float64 and then to fp32 (a true fma
    rounds once; the two differ only where the float64 sum lies within 2^-29 ulp of an fp32 tie)"""
    return (np.float64(g) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _chain(v, g32, axis):
    """the kernel's tap chain along ``axis`` of fp32 ``v``: fl(g_0 v_0), then fma(g_k, v_k, acc) for k = 1..10"""
    n = v.shape[axis] - TAPS + 1
    take = lambda k: np.take(v, np.arange(k, k + n), axis=axis)  # noqa: E731
    acc = g32[0] * take(0)
    for k in range(1, TAPS):
        acc = _fma(g32[k], take(k), acc)
    return acc


def emulate(a, b, tile=TILE):
    """the kernel's arithmetic in numpy fp32, operation by operation (module docstring) -> map [H-10, W-10, C] fp32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    h, w, c = a.shape
    g32 = window().astype(np.float32)
    r = data_range(a, b)
    c1, c2 = np.float32((K1 * r) ** 2), np.float32((K2 * r) ** 2)
    out = np.zeros((h - TAPS + 1, w - TAPS + 1, c), np.float32)
    two = np.float32(2.0)
    for y0, x0, py, px in tiles(h, w, tile):
        p, q = a[py, px], b[py, px]
        sa, sb = _halo(a, y0, x0, p, tile), _halo(b, y0, x0, q, tile)
        ma, mb, maa, mbb, mab = (_chain(_chain(v, g32, 1), g32, 0) for v in (sa, sb, sa * sa, sb * sb, sa * sb))
        mua, mub = p + ma, q + mb
        var_a, var_b, cov = maa - ma * ma, mbb - mb * mb, mab - ma * mb
        with np.errstate(invalid="ignore", divide="ignore"):
            s = ((two * (mua * mub) + c1) * (two * cov + c2)) / (((mua * mua + mub * mub) + c1) * ((var_a + var_b) + c2))
        assert s.dtype == np.float32
        part = out[y0:y0 + tile, x0:x0 + tile]
        part[...] = s[:part.shape[0], :part.shape[1]]
    return out


class _V:
    """a float64 value with a bound on its absolute error; every operation adds the rounding u |result|"""

    def __init__(self, v, e):
        self.v, self.e = v, e

    @staticmethod
    def _rounded(v, e):
        return _V(v, e + U * np.abs(v))

    def __add__(self, o):
        return _V._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return _V._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return _V._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        v = self.v / o.v
        return _V._rounded(v, self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v))

    def twice(self):
        return _V(2 * self.v, 2 * self.e)


def window_bound(a, b, tile=TILE):
    """B [H-10, W-10, C]: the bound on |kernel's s - float64 s| per window (module docstring)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    h, w, c = a.shape
    g = window()
    r = data_range(a, b)
    c1, c2 = (K1 * r) ** 2, (K2 * r) ** 2
    out = np.zeros((h - TAPS + 1, w - TAPS + 1, c))
    for y0, x0, py, px in tiles(h, w, tile):
        p, q = a[py, px], b[py, px]
        sa, sb = _halo(a, y0, x0, p, tile).astype(np.float64), _halo(b, y0, x0, q, tile).astype(np.float64)
        lin = lambda v: _V(_blur(v, g), K_LIN * U * _blur(np.abs(v), g))  # noqa: E731
        quad = lambda v: _V(_blur(v, g), K_QUAD * U * _blur(np.abs(v), g))  # noqa: E731
        ma, mb, maa, mbb, mab = lin(sa), lin(sb), quad(sa * sa), quad(sb * sb), quad(sa * sb)
        exact = lambda v: _V(np.broadcast_to(np.asarray(v, np.float64), ma.v.shape), 0.0)  # noqa: E731
        k1, k2 = _V(np.full_like(ma.v, c1), U * c1), _V(np.full_like(ma.v, c2), U * c2)
        mua, mub = exact(p) + ma, exact(q) + mb
        var_a, var_b, cov = maa - ma * ma, mbb - mb * mb, mab - ma * mb
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (((mua * mub).twice() + k1) * (cov.twice() + k2)) / (((mua * mua + mub * mub) + k1) * ((var_a + var_b) + k2))
        part = out[y0:y0 + tile, x0:x0 + tile]
        part[...] = s.e[:part.shape[0], :part.shape[1]]
    return out


# ---- test images --------------------------------------------------------------------------------------------------------
def images(kind, h, w, c=3, seed=900):
    """(a, b) fp32 [h, w, c]: ``noise`` uniform noise and a perturbed copy; ``smooth`` a sinusoid and itself plus 2 % noise;
    ``flat`` 0.7 +- 1e-3 with one 0 and one 1 pixel (R = 1); ``dark`` values <= 0.02"""
    shape = (h, w, c)
    if kind == "noise":
        a = synth.uniform(shape, 0.0, 1.0, seed)
        b = np.clip(a + 0.1 * synth.normal(shape, seed + 1), 0.0, 1.0)
    elif kind == "smooth":
        y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
        a = 0.5 + 0.4 * np.sin(2 * np.pi * (y / 37.0 + x / 53.0) + 0.7 * ch) * np.cos(2 * np.pi * x / 91.0)
        b = a + 0.02 * synth.normal(shape, seed + 2)
    elif kind == "flat":
        a = 0.7 + synth.uniform(shape, -1e-3, 1e-3, seed + 3)
        b = 0.7 + synth.uniform(shape, -1e-3, 1e-3, seed + 4)
        a[h // 3, w // 3, 0], a[2 * h // 3, 2 * w // 3, 0] = 0.0, 1.0
    elif kind == "dark":
        a = synth.uniform(shape, 0.0, 0.02, seed + 5)
        b = np.clip(a + 0.002 * synth.normal(shape, seed + 6), 0.0, 0.02)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


_cases = {}


def case(kind, h, w, c=3):
    """(a, b, float64 map, B) of a test image: computed once per process, shared, read-only"""
    key = (kind, h, w, c)
    if key not in _cases:
        a, b = range_pair(h, w, c) if kind == "range" else images(kind, h, w, c)
        _cases[key] = (a, b, ssim_valid(a, b), window_bound(a, b))
        for x in _cases[key]:
            x.setflags(write=False)
    return _cases[key]


def sizes(tile=TILE):
    """one window; one row / column of windows; one window short of, at and past a tile edge in each direction; several
    ragged tiles"""
    t = tile
    return [(11, 11), (11, 12), (12, 11), (t + 9, t + 10), (t + 10, t + 11), (t + 11, t + 9), (2 * t + 13, t + 17), (96, 160)]


def range_pair(h, w, c=3, seed=950):
    """a in [0.2, 0.6], b in [0, 1], both attaining their ends: R comes from b"""
    a = synth.uniform((h, w, c), 0.2, 0.6, seed).astype(np.float32)
    b = synth.uniform((h, w, c), 0.0, 1.0, seed + 1).astype(np.float32)
    a[1, 2, 0], a[3, 4, 0], b[5, 6, 0], b[7, 8, 0] = 0.2, 0.6, 0.0, 1.0
    return a, b
