"""References for LPIPS (csrc/lpips.hip, ops_lpips.py, model_components/lpips.py): the float64 restatement of the metric
in plain torch, an fp16-operand emulation of the kernels' arithmetic, seeded weights under the documented state-dict keys, a
stand-in for the reference's module tree, exact-integer operand builders for the convolutions and the bounds of the head.
Shared by tests/test_lpips_host.py, test_gpu_lpips_kernels.py, test_gpu_lpips.py and scripts/bench_lpips.py; computes
nothing on a GPU.

The metric (torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True), restated from memory of
its source -- UNVERIFIED against the package, which is not available where this was written):
  x = 2 img - 1;  x = (x - shift) / scale;  AlexNet features tapped after each ReLU;  n(f) = f / sqrt(eps + sum_c f_c^2)
  (EPS_INSIDE; the original `lpips` package has f / (sqrt(sum_c f_c^2) + 1e-10): EPS_OUTSIDE);
  d_k = sum_c lin_k[c] (n(fa)_c - n(fb)_c)^2;  lpips = sum_k mean_pixels d_k per pair, then the mean over the batch.

Why integers make the convolution tests exact: see vgg_refs.py -- operands in {-2..2}, sum |a||w| + |bias| <= 2048 at every
output, so any fp32 summation order gives the same integer, which fp16 holds."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from vgg_refs import assert_equal, assert_exact_operands, nchw, nhwc, round16  # noqa: F401  (re-exported)

IMAGE_CHANNELS = 4  # NRHIP_LPIPS_IMAGE_CHANNELS
U32 = 2.0 ** -24
U16 = 2.0 ** -11
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS_INSIDE, EPS_OUTSIDE = 0, 1
EPS = {EPS_INSIDE: 1e-8, EPS_OUTSIDE: 1e-10}
# (pool before the convolution, cin, cout, kernel, stride, pad, torchvision's index of the convolution in alexnet().features)
LAYERS = ((False, 3, 64, 11, 4, 2, 0), (True, 64, 192, 5, 1, 2, 3), (True, 192, 384, 3, 1, 1, 6), (False, 384, 256, 3, 1, 1, 8),
          (False, 256, 256, 3, 1, 1, 10))
CONV_SHAPES = tuple(l[1:6] for l in LAYERS)
TAP_CHANNELS = tuple(l[2] for l in LAYERS)
MIN_SIZE = 31
TOL = 5e-4    # end to end, absolute (LPIPS is published to three decimals)
FLOOR = 5e-3  # every end-to-end case but the identical pair has a float64 value above this


def stored(c):
    return IMAGE_CHANNELS if c == 3 else c


def state_dict_keys():
    keys = ["net.scaling_layer.shift", "net.scaling_layer.scale"]
    for k, l in enumerate(LAYERS):
        keys += [f"net.net.slice{k + 1}.{l[6]}.weight", f"net.net.slice{k + 1}.{l[6]}.bias"]
    return keys + [f"net.lin{k}.model.1.weight" for k in range(5)]


def make_weights(seed=0):
    """-> OrderedDict key -> fp32 tensor: He-scaled normal convolution weights rounded to fp16, biases of about 0.05, lin
    weights uniform in [0, 1) (non-negative, as the trained ones are)"""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    sd["net.scaling_layer.shift"] = torch.tensor(SHIFT).reshape(1, 3, 1, 1)
    sd["net.scaling_layer.scale"] = torch.tensor(SCALE).reshape(1, 3, 1, 1)
    for k, (_, cin, cout, ks, _, _, idx) in enumerate(LAYERS):
        w = torch.randn((cout, cin, ks, ks), generator=g) * math.sqrt(2.0 / (ks * ks * cin))
        b = 0.05 + 0.02 * torch.randn((cout,), generator=g)
        sd[f"net.net.slice{k + 1}.{idx}.weight"] = w.half().float()
        sd[f"net.net.slice{k + 1}.{idx}.bias"] = b.half().float()
    for k, c in enumerate(TAP_CHANNELS):
        sd[f"net.lin{k}.model.1.weight"] = torch.rand((1, c, 1, 1), generator=g)
    return OrderedDict((k, sd[k]) for k in state_dict_keys())


CONTENTS = ("noise", "same", "near")
E2E_SIZES = ((31, 31), (35, 47), (67, 131))


def make_pair(b, h, w, content, seed=1):
    """two NCHW [b, 3, h, w] fp32 images in [0, 1]: independent noise; an image and itself; an image and a copy perturbed
    by +-0.04 per value (the regime of a rendered image against its ground truth)"""
    g = torch.Generator().manual_seed(seed + 1000 * h + w)
    x = torch.rand((b, 3, h, w), generator=g)
    if content == "noise":
        return x, torch.rand((b, 3, h, w), generator=g)
    if content == "same":
        return x, x.clone()
    return x, (x + 0.08 * (torch.rand((b, 3, h, w), generator=g) - 0.5)).clamp(0, 1)


# ---- the metric ------------------------------------------------------------------------------------------------------------
def stage_ref(img_nchw, shift=SHIFT, scale=SCALE):
    """step 1 in float64; shift and scale are the fp32 parameters"""
    sh = torch.tensor(shift, dtype=torch.float32).double().reshape(1, 3, 1, 1)
    sc = torch.tensor(scale, dtype=torch.float32).double().reshape(1, 3, 1, 1)
    return ((2.0 * img_nchw.double() - 1.0) - sh) / sc


def normalize_ref(f, eps_mode=EPS_INSIDE, eps=None):
    eps = EPS[eps_mode] if eps is None else eps
    s = (f * f).sum(dim=1, keepdim=True)
    return f / torch.sqrt(eps + s) if eps_mode == EPS_INSIDE else f / (torch.sqrt(s) + eps)


def head_ref(fa, fb, lin, eps_mode=EPS_INSIDE, eps=None):
    """NCHW features of one tap -> [B] float64: mean over pixels of sum_c lin_c (n(fa)_c - n(fb)_c)^2"""
    d = (normalize_ref(fa.double(), eps_mode, eps) - normalize_ref(fb.double(), eps_mode, eps)) ** 2
    return (d * lin.double().reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def features_ref(x, sd, dtype=torch.float64, emulate=False):
    """AlexNet taps of a staged NCHW batch.  emulate: the kernels' number formats -- the staged image, the weights and every
    stored activation rounded to fp16; products and sums stay in ``dtype`` (float64: an upper bound on what fp32
    accumulation keeps), bias added unrounded"""
    rnd = (lambda t: t.float().half().to(dtype)) if emulate else (lambda t: t)
    x, taps = rnd(x.to(dtype)), []
    for k, (pool, _, _, _, stride, pad, idx) in enumerate(LAYERS):
        if pool:
            x = F.max_pool2d(x, 3, 2)
        w, b = sd[f"net.net.slice{k + 1}.{idx}.weight"].to(dtype), sd[f"net.net.slice{k + 1}.{idx}.bias"].to(dtype)
        x = rnd(F.conv2d(x, rnd(w), b, stride=stride, padding=pad).clamp_min(0))
        taps.append(x)
    return taps


def lpips_pairs_ref(a, b, sd, eps_mode=EPS_INSIDE, dtype=torch.float64, emulate=False):
    """-> [B] per-pair values (float64 unless ``dtype`` says otherwise)"""
    n = a.shape[0]
    if dtype == torch.float64:
        x = stage_ref(torch.cat([a, b]), sd["net.scaling_layer.shift"].flatten().tolist(),
                      sd["net.scaling_layer.scale"].flatten().tolist())
    else:
        x = (2 * torch.cat([a, b]).to(dtype) - 1 - sd["net.scaling_layer.shift"].to(dtype)) / sd["net.scaling_layer.scale"].to(dtype)
    total = 0
    for k, f in enumerate(features_ref(x, sd, dtype, emulate)):
        lin = sd[f"net.lin{k}.model.1.weight"].to(dtype)
        if dtype == torch.float64:
            total = total + head_ref(f[:n], f[n:], lin, eps_mode)
        else:
            na, nb = normalize_ref(f[:n], eps_mode), normalize_ref(f[n:], eps_mode)
            total = total + (((na - nb) ** 2) * lin.reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))
    return total


def lpips_ref(a, b, sd, eps_mode=EPS_INSIDE):
    return float(lpips_pairs_ref(a, b, sd, eps_mode).mean())


# ---- a stand-in for the reference's object ------------------------------------------------------------------------------------
class _StandInScaling(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE)[None, :, None, None])


class _StandInAlex(torch.nn.Module):
    """built the way the LPIPS packages build theirs: ONE torchvision-style ``features`` Sequential, its layers added to
    five slices under their own indices"""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        feats = nn.Sequential(nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2), nn.Conv2d(64, 192, 5, padding=2),
                              nn.ReLU(inplace=True), nn.MaxPool2d(3, 2), nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True),
                              nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(256, 256, 3, padding=1),
                              nn.ReLU(inplace=True))
        for k, (a, b) in enumerate(((0, 2), (2, 5), (5, 8), (8, 10), (10, 12))):
            sl = nn.Sequential()
            for i in range(a, b):
                sl.add_module(str(i), feats[i])
            setattr(self, f"slice{k + 1}", sl)


class _StandInLin(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.model = torch.nn.Sequential(torch.nn.Dropout(), torch.nn.Conv2d(c, 1, 1, bias=False))


class _StandInNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.scaling_layer = _StandInScaling()
        self.net = _StandInAlex()
        for k, c in enumerate(TAP_CHANNELS):
            setattr(self, f"lin{k}", _StandInLin(c))


class ReferenceStyleLPIPS(torch.nn.Module):
    """a stand-in with the attributes LPIPS.from_reference reads from the reference model's ``self.lpips``: ``net`` and
    ``normalize``"""

    def __init__(self, normalize=True):
        super().__init__()
        self.net = _StandInNet().eval()
        self.net.requires_grad_(False)
        self.normalize = normalize


# ---- kernels: exact convolution cases ------------------------------------------------------------------------------------------
def out_size(n, ks, stride, pad):
    return (n + 2 * pad - ks) // stride + 1


def _sparse_ints(shape, density, g):
    v = torch.randint(-2, 3, shape, generator=g).double()
    return v * (torch.rand(shape, generator=g) < density).double()


def conv_case(b, h, w, layer, seed, border=False):
    """operands (NHWC fp16 input with the stored channel count, fp32 weight and bias) and the float64 result of
    relu(conv + bias) rounded to fp16, for CONV_SHAPES[layer].  border: every border pixel of the input is non-zero in
    every real channel.  Every case has negative pre-activations (asserted), so the ReLU acts."""
    cin, cout, ks, stride, pad = CONV_SHAPES[layer]
    g = torch.Generator().manual_seed(seed)
    dens = 0.5 if cin == 3 else 0.25
    wt = _sparse_ints((cout, cin, ks, ks), dens, g)
    bias = torch.randint(-3, 4, (cout,), generator=g).double()
    x = _sparse_ints((b, cin, h, w), dens, g)
    if border:
        edge = torch.zeros((h, w), dtype=torch.bool)
        edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
        sign = torch.where(torch.rand((b, cin, h, w), generator=g) < 0.5, -1.0, 1.0).double()
        x = torch.where(edge & (x == 0), sign, x)
        assert bool((x[:, :, edge] != 0).all())
    assert_exact_operands(F.conv2d(x.abs(), wt.abs(), bias.abs(), stride=stride, padding=pad))
    pre = F.conv2d(x, wt, bias, stride=stride, padding=pad)
    assert float(pre.min()) < 0 < float(pre.max())
    xs = nhwc(x)
    if stored(cin) != cin:
        xs = torch.cat([xs, torch.zeros(xs.shape[:3] + (stored(cin) - cin,), dtype=xs.dtype)], dim=-1)
    return {"x": xs.half(), "w": wt.float(), "bias": bias.float(), "out": nhwc(pre.clamp_min(0)).half()}


def conv_case_sizes(layer):
    """(B, H, W) of the exact cases: for conv1 35 x 47 (8 x 11 outputs) and 31 x 31 (7 x 7), for the others 8 x 11 and 1 x 1
    maps, with B = 1 and B = 3 (3 * 88 = 264 and 3 * 49 = 147 output pixels: tiles of 32 and 64 cross rows and images).  At 35,
    47 and 31 the last stride-4 window ends exactly on the padded edge ((n + 4 - 11) % 4 == 0), so conv1 gets 33 x 38 as
    well: (33 + 4 - 11) % 4 = 2 rows and (38 + 4 - 11) % 4 = 3 columns are never the last tap of any window"""
    sizes = ((35, 47), (31, 31)) if layer == 0 else ((8, 11), (1, 1))
    return [(b, h, w) for (h, w) in sizes for b in (1, 3)] + ([(2, 33, 38)] if layer == 0 else [])


def pool_ref(x_nhwc):
    return nhwc(F.max_pool2d(nchw(x_nhwc.float()), 3, 2)).half()


# ---- kernels: the head -----------------------------------------------------------------------------------------------------------
def head_case(b, pixels, c, seed, zero_both=True, zero_one=True):
    """fp16 features [2 b, pixels, c] (non-negative, as after a ReLU, a third of them zero) and lin [c] >= 0; pixel 0 of
    pair 0 is all zero in both images (zero_both), the last pixel of the last pair in the second image only (zero_one)"""
    g = torch.Generator().manual_seed(seed)
    f = (torch.randn((2 * b, pixels, c), generator=g).clamp_min(0) * 2 + (torch.rand((2 * b, pixels, c), generator=g) < 0.2)).half()
    if zero_both:
        f[0, 0], f[b, 0] = 0, 0
    if zero_one:
        f[2 * b - 1, pixels - 1] = 0
        f[b - 1, pixels - 1, 0] = 1.0
    return f, torch.rand((c,), generator=g)


def head_pixels_ref(f, lin, eps_mode, eps=None):
    """-> (d [B, pixels] float64, bound [B, pixels]) for features [2 B, pixels, C].  The bound of a kernel that works in fp32
    with correctly rounded sqrt and division, u = 2^-24: the sum of C non-negative squares carries at most (C + 1) u
    relative, its root half of that plus u, eps' addition u, the division u: r = (C / 2 + 4) u relative on every normalised
    value.  delta = na - nb then has |err| <= r (|na| + |nb|) + u |delta|; its square 2 |delta| |err| + u delta^2 (+ second
    order); times lin and summed over C terms adds (C + 1) u of sum |lin| delta^2."""
    b = f.shape[0] // 2
    c = f.shape[-1]
    fa, fb = f[:b].double().permute(0, 2, 1)[..., None], f[b:].double().permute(0, 2, 1)[..., None]  # [B, C, pixels, 1]
    na, nb = normalize_ref(fa, eps_mode, eps), normalize_ref(fb, eps_mode, eps)
    l = lin.double().abs().reshape(1, -1, 1, 1)
    delta = na - nb
    r = (c / 2 + 4) * U32
    err = r * (na.abs() + nb.abs()) + U32 * delta.abs()
    bound = (l * (2 * delta.abs() * err + err * err + (c + 2) * U32 * delta * delta)).sum(dim=1)[..., 0]
    d = (lin.double().reshape(1, -1, 1, 1) * delta * delta).sum(dim=1)[..., 0]
    return d, bound


def head_out_ref(f, lin, eps_mode, eps=None, accum=None):
    """-> (out [B] float64, bound [B]): the mean over pixels (float64 in the kernel: nothing to add) and the one rounding
    to fp32 of (accum +) mean"""
    d, bound = head_pixels_ref(f, lin, eps_mode, eps)
    out = d.mean(dim=1) + (0 if accum is None else accum.double())
    return out, bound.mean(dim=1) + U32 * out.abs()


# ---- emulation -------------------------------------------------------------------------------------------------------------------
def emulation_table(seed=0):
    """-> rows (case, float64 value, |fp16-operand emulation - float64|, |fp32 torch - float64|), worst pair of each case"""
    sd = make_weights(seed)
    rows = []
    for (h, w) in E2E_SIZES:
        for b in (1, 2):
            for content in CONTENTS:
                x, y = make_pair(b, h, w, content)
                ref = lpips_pairs_ref(x, y, sd)
                emu = lpips_pairs_ref(x, y, sd, emulate=True)
                f32 = lpips_pairs_ref(x, y, sd, dtype=torch.float32).double()
                rows.append((f"{h}x{w} B={b} {content}", float(ref.min()), float((emu - ref).abs().max()),
                             float((f32 - ref).abs().max())))
    return rows


if __name__ == "__main__":
    for row in emulation_table():
        print("%-22s ref %.6f  fp16-emulated %.2e  fp32 %.2e" % row)
