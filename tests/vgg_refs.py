"""References for the VGG perceptual loss (csrc/vgg_loss.hip, model_components/perceptual.py): float64 restatements of
every kernel, exact-integer operand builders, the network's layer list, seeded weights, and the float64 backward chain on a
node's own saved tensors.  Shared by tests/test_gpu_vgg_kernels.py, test_gpu_vgg_loss.py, test_vgg_loss_host.py and
scripts/bench_vgg_loss.py; computes nothing on a GPU.

Why integers make the convolution exact: operands in {-2..2} are fp16 values, every product is an integer of magnitude <= 4,
and `assert_exact_operands` checks that sum |a| |w| (+ |bias|) <= 2048 at every output -- so every partial sum, in ANY order,
is an integer below 2^24 (exact in fp32) and the result an integer of magnitude <= 2048 (exact in fp16)."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

IMAGE_CHANNELS = 16
U32 = 2.0 ** -24   # fp32 unit roundoff
U16 = 2.0 ** -11   # fp16 unit roundoff
LAYOUT = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512)
CUTS = ((0, 2), (2, 7), (7, 12), (12, 21), (21, 30))
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)  # torchvision's index in vgg19().features
TAP_WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
CHANNEL_PAIRS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512))


def stored(c):
    return IMAGE_CHANNELS if c == 3 else c


def steps():
    """-> [("conv", src, dst, cin, cout) | ("pool", src, dst) | ("tap", src, i)], the order the node runs them in"""
    out, cur, cin, block, within, tap = [], "image", 3, 1, 0, 0
    for v in LAYOUT:
        if v == "M":
            out.append(("pool", cur, f"pool{block}"))
            cur, block, within = f"pool{block}", block + 1, 0
        else:
            within += 1
            dst = f"conv{block}_{within}"
            out.append(("conv", cur, dst, cin, v))
            cur, cin = dst, v
            if within == 1:
                out.append(("tap", cur, tap))
                tap += 1
    return out


def state_dict_keys():
    keys = []
    for k, (a, b) in enumerate(CUTS):
        for i in CONV_INDEX:
            if a <= i < b:
                keys += [f"vgg.slice{k + 1}.0.{i}.weight", f"vgg.slice{k + 1}.0.{i}.bias"]
    return keys


def key_of(conv_name, leaf):
    i = CONV_INDEX[[s[2] for s in steps() if s[0] == "conv"].index(conv_name)]
    k = next(k for k, (a, b) in enumerate(CUTS) if a <= i < b)
    return f"vgg.slice{k + 1}.0.{i}.{leaf}"


class ReferenceStyleVgg(torch.nn.Module):
    """a stand-in built the way the reference builds its network: ONE Sequential in torchvision's "E" layout, sliced with
    [:2], [2:7], [7:12], [12:21], [21:30], every slice wrapped in a Sequential"""

    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for v in LAYOUT:
            if v == "M":
                layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [torch.nn.Conv2d(cin, v, kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
                cin = v
        features = torch.nn.Sequential(*layers)
        for k, (a, b) in enumerate(CUTS):
            setattr(self, f"slice{k + 1}", torch.nn.Sequential(features[a:b]))

    def forward(self, x):
        out = []
        for k in range(5):
            x = getattr(self, f"slice{k + 1}")(x)
            out.append(x)
        return out


class ReferenceStyleLoss(torch.nn.Module):
    """the restated torch network with the reference module's attributes (vgg, weights) and call signature"""

    def __init__(self, weights=None):
        super().__init__()
        self.vgg = ReferenceStyleVgg().eval()
        self.vgg.requires_grad_(False)
        self.weights = list(TAP_WEIGHTS if weights is None else weights)

    def forward(self, x, y):
        feats = self.vgg(torch.cat([x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)], dim=0))
        loss = 0
        for w, f in zip(self.weights, feats):
            fx, fy = f.chunk(2, dim=0)
            loss = loss + w * F.l1_loss(fx, fy.detach())
        return loss


def make_weights(seed=0):
    """-> OrderedDict state-dict key -> fp32 tensor: He-scaled normal weights rounded to fp16, biases of about 0.05"""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for st in steps():
        if st[0] != "conv":
            continue
        _, _, dst, cin, cout = st
        w = torch.randn((cout, cin, 3, 3), generator=g) * math.sqrt(2.0 / (9 * cin))
        b = 0.05 + 0.02 * torch.randn((cout,), generator=g)
        sd[key_of(dst, "weight")] = w.half().float()
        sd[key_of(dst, "bias")] = b.half().float()
    return sd


def make_images(b, h, w, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((b, h, w, 3), generator=g).half().float()
    y = (x + 0.25 * (torch.rand((b, h, w, 3), generator=g) - 0.5)).clamp(0, 1).half().float()
    return x, y


# ---- layouts ------------------------------------------------------------------------------------------------------------
def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the convolution on exact integers ------------------------------------------------------------------------------------
def _sparse_ints(shape, density, lo, hi, g):
    v = torch.randint(lo, hi + 1, shape, generator=g).double()
    return v * (torch.rand(shape, generator=g) < density).double()


def conv_shapes(pixel_blocks):
    """(B, H, W) for a wave tile of T = 32 * pixel_blocks pixels of the flattened batch: one pixel; one ragged tile (T - 1
    pixels, as one row and as one column); two tiles with a single pixel in the second (a row, a column); 6 x 6 with B = 3
    (108 pixels: tiles cross the image boundaries); two images of an odd size"""
    t = 32 * pixel_blocks
    return [(1, 1, 1), (1, 1, t - 1), (1, t - 1, 1), (1, 1, t + 1), (1, t + 1, 1), (3, 6, 6), (2, 5, 7)]


def conv_case(b, h, w, cin, cout, seed, mode=None):
    """operands and float64 results of one Conv2d(cin, cout, 3, padding=1), NHWC, the image side stored with IMAGE_CHANNELS
    channels.  mode 0: forward (x, w, bias -> out); mode 1: input gradient (g, w, act -> gx); None: both"""
    g = torch.Generator().manual_seed(seed)
    dens = 0.5 if max(cin, cout) <= 64 else 0.25
    wt = _sparse_ints((cout, cin, 3, 3), dens, -2, 2, g)
    bias = torch.randint(-3, 4, (cout,), generator=g).double()

    def pad(t, c):  # NCHW float64 -> NHWC fp16 with the stored channel count
        t = nhwc(t)
        if stored(c) != c:
            t = torch.cat([t, torch.zeros(t.shape[:3] + (stored(c) - c,), dtype=t.dtype)], dim=-1)
        return t.half()

    case = {"w": wt.float(), "bias": bias.float()}
    if mode in (None, 0):
        x = _sparse_ints((b, cin, h, w), dens, -2, 2, g)
        assert_exact_operands(F.conv2d(x.abs(), wt.abs(), bias.abs(), padding=1))
        case.update(x=pad(x, cin), out=pad(F.conv2d(x, wt, bias, padding=1).clamp_min(0), cout))
    if mode in (None, 1):
        gy = _sparse_ints((b, cout, h, w), dens, -2, 2, g)
        act = torch.randint(-1, 3, (b, cin, h, w), generator=g).double()  # the layer's stored input: a quarter <= 0
        assert_exact_operands(F.conv_transpose2d(gy.abs(), wt.abs(), padding=1))
        gx = F.conv_transpose2d(gy, wt, padding=1)
        if cin != 3:  # (no mask on the gradient that reaches the image)
            gx = gx * (act > 0)
        case.update(g=pad(gy, cout), act=pad(act, cin), gx=pad(gx, cin))
    return case


def assert_exact_operands(*abs_sums):
    for s in abs_sums:
        assert float(s.max()) <= 2048.0, f"operands too dense: sum |a||w| reaches {float(s.max())}"


def assert_equal(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert not torch.isnan(got.float()).any(), f"{what}: {int(torch.isnan(got.float()).sum())} elements unwritten (NaN prefill)"
    bad = got.double() != want.double()
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


# ---- maxpool ------------------------------------------------------------------------------------------------------------
def pool_windows(x):
    """NHWC [B, H, W, C] -> [B, H//2, W//2, C, 4] windows in row-major order (floor mode)"""
    b, h, w, c = x.shape
    ho, wo = h // 2, w // 2
    x = x[:, :2 * ho, :2 * wo]
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], dim=-1)


def pool_first_argmax(x):
    win = pool_windows(x.double())
    best, arg = win[..., 0], torch.zeros(win.shape[:-1], dtype=torch.long)
    for k in range(1, 4):
        upd = win[..., k] > best
        best, arg = torch.where(upd, win[..., k], best), torch.where(upd, torch.full_like(arg, k), arg)
    return best, arg


def pool_fwd(x):
    return pool_first_argmax(x)[0]


def pool_bwd(x, g):
    """gradient of pool_fwd w.r.t. x (float64): g at the first maximum of every window, zero elsewhere and in a dropped odd
    row / column"""
    b, h, w, c = x.shape
    _, arg = pool_first_argmax(x)
    out = torch.zeros((b, h, w, c), dtype=torch.float64)
    for k in range(4):
        out[:, (k >> 1):2 * (h // 2):2, (k & 1):2 * (w // 2):2] = torch.where(arg == k, g.double(), torch.zeros((), dtype=torch.float64))
    return out


# ---- working scale ------------------------------------------------------------------------------------------------------
def pow2_norm(amax):
    """the power of two p with amax * p in [0.5, 1); 1 for 0 (the kernels' rule)"""
    if amax == 0:
        return 1.0
    return 2.0 ** -math.frexp(float(amax))[1]


def round16(t):
    return t.float().half().double()


# ---- the network on a node's own saved tensors ----------------------------------------------------------------------------
def conv_layer_ref(a_nhwc, w, bias):
    """float64 relu(conv + bias) of a stored fp16 input and the bound of a fp32-accumulating kernel on it, per element:
    (9 Cin + 1) u sum |a||w| + 2^-11 |ref| (every one of the 9 Cin products and the bias enters a running fp32 sum whose
    magnitude never exceeds sum |a||w|: at most one rounding each; then one rounding to fp16)"""
    cin = w.shape[1]
    a = nchw(a_nhwc.double())[:, :cin]
    w, bias = w.double(), bias.double()
    ref = F.conv2d(a, w, bias, padding=1).clamp_min(0)
    mag = F.conv2d(a.abs(), w.abs(), bias.abs(), padding=1)
    bound = (9 * cin + 1) * U32 * mag + U16 * ref.abs()
    return nhwc(ref), nhwc(bound)


def loss_ref(saved, b, tap_weights=TAP_WEIGHTS):
    total = 0.0
    for st in steps():
        if st[0] == "tap":
            f = saved[st[1]].double()
            total += tap_weights[st[2]] * float((f[:b] - f[b:]).abs().mean())
    return total


def backward_ref(saved, weights, b, g=1.0, tap_weights=TAP_WEIGHTS, rounded=False):
    """float64 gradient of the loss w.r.t. x [B, H, W, 3], linearised on the node's saved tensors (ReLU masks and pool argmax
    from the saved activations, L1 signs from the saved features).  rounded=True: every inter-layer gradient is rounded to
    fp16 at the power-of-two scale the kernels' rule gives it (a tensor is (stored, S), stored = S * true)."""
    rnd = round16 if rounded else (lambda t: t)
    grads = {}  # name -> (stored float64 NHWC, S)
    for st in reversed(steps()):
        if st[0] == "tap":
            f = saved[st[1]].double()
            fx, fy = f[:b], f[b:]
            c = tap_weights[st[2]] * g / fx.numel()
            term = torch.sign(fx - fy) * (fx > 0)
            if st[1] in grads:
                above, s_a = grads.pop(st[1])
                s_out = pow2_norm(abs(c) + float(above.abs().max()) / s_a)
                grads[st[1]] = (rnd(term * (c * s_out) + above * (s_out / s_a)), s_out)
            else:
                s_out = pow2_norm(abs(c))
                grads[st[1]] = (rnd(term * (c * s_out)), s_out)
        elif st[0] == "conv":
            _, src, dst, cin, cout = st
            gy, s_in = grads.pop(dst)
            p = pow2_norm(float(gy.abs().max()))
            gx = nhwc(F.conv_transpose2d(nchw(gy), weights[key_of(dst, "weight")].double(), padding=1)) * p
            if src != "image":
                gx = gx * (saved[src][:b] > 0)
            grads[src] = (rnd(gx), s_in * p)
        else:
            _, src, dst = st
            gy, s_in = grads.pop(dst)
            p = pow2_norm(float(gy.abs().max()))
            grads[src] = (pool_bwd(saved[src][:b], gy * p), s_in * p)
    gx, s = grads["image"]
    return gx / s


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
