"""LPIPS, the third image metric of the reference's ``get_image_metrics_and_images`` (``self.lpips =
LearnedPerceptualImagePatchSimilarity(normalize=True)``, models/neurad.py:267, called at 587): torchmetrics >= 1.0.1 with
``net_type="alex"`` and ``reduction="mean"``.  For two images a, b [B, 3, H, W] in [0, 1]:

  1. x = 2 img - 1, then (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450);
  2. AlexNet features tapped after each ReLU: conv 3->64 k11 s4 p2 | pool(3, 2), conv 64->192 k5 p2 | pool(3, 2), conv
     192->384 k3 p1 | conv 384->256 k3 p1 | conv 256->256 k3 p1; every convolution has a bias, pools floor without padding;
  3. per tap k and pixel n(f) = f / sqrt(eps + sum_c f_c^2), eps = 1e-8; d_k = sum_c lin_k[c] (n(fa)_c - n(fb)_c)^2 with
     lin_k the tap's bias-free 1 x 1 convolution;
  4. lpips = sum_k mean_pixels d_k per pair; the module returns the mean over the batch.

UNVERIFIED on the machine this was written on: neither torchmetrics nor torchvision was available there, so the formula,
the placement of eps and the state-dict names below are restated from memory of torchmetrics' source.  The original
``lpips`` package normalises with f / (sqrt(sum f^2) + 1e-10); ``eps_mode`` / ``eps`` select between the two, down to an
argument of the head kernel, so a mismatch is a one-line fix.  The kernels have only been run with seeded weights.

On a GPU the metric is one launch sequence of csrc/lpips.hip (ops_lpips.py): a staging kernel that also raises the
value-range flag torchmetrics pays a host read for, five convolutions on the fp16 matrix cores (fp32 accumulation), two
pools, five head kernels with float64 sums in a fixed order.  Nothing is read back by ``forward``.  On any other device
the same module runs its own ``nn.Conv2d`` layers: there is no second implementation.

State-dict keys (torchmetrics' object, as remembered): ``net.scaling_layer.{shift,scale}``,
``net.net.slice{1..5}.{0,3,6,8,10}.{weight,bias}``, ``net.lin{0..4}.model.1.weight``.  The step program is read off the
module tree, not off these names, so ``from_reference`` adopts the reference's object whatever its exact names are."""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Tuple

import torch
from torch import Tensor, nn

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS_INSIDE, EPS_OUTSIDE = 0, 1  # _lib.LPIPS_EPS_*
DEFAULT_EPS = {EPS_INSIDE: 1e-8, EPS_OUTSIDE: 1e-10}
MIN_SIZE = 31  # below it the second pool is empty
TAP_CHANNELS = (64, 192, 384, 256, 256)
# torchvision's alexnet().features[:12], cut after each ReLU
_CUTS = ((0, 2), (2, 5), (5, 8), (8, 10), (10, 12))


def _feature_layers() -> List[nn.Module]:
    return [nn.Conv2d(3, 64, 11, stride=4, padding=2), nn.ReLU(inplace=False), nn.MaxPool2d(3, 2),
            nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=False), nn.MaxPool2d(3, 2),
            nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=False), nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=False),
            nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=False)]


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE)[None, :, None, None])

    def forward(self, x: Tensor) -> Tensor:
        return (x - self.shift) / self.scale


class AlexSlices(nn.Module):
    """the five feature slices, every layer under torchvision's own index"""

    def __init__(self):
        super().__init__()
        layers = _feature_layers()
        for k, (a, b) in enumerate(_CUTS):
            setattr(self, f"slice{k + 1}", nn.Sequential(OrderedDict((str(i), layers[i]) for i in range(a, b))))


class NetLinLayer(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(channels, 1, 1, bias=False))


class LpipsNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.net = AlexSlices()
        for k, c in enumerate(TAP_CHANNELS):
            setattr(self, f"lin{k}", NetLinLayer(c))


def _conv_shape(m: nn.Conv2d) -> Tuple[int, int, int, int, int]:
    if (m.kernel_size[0] != m.kernel_size[1] or m.stride[0] != m.stride[1] or m.padding[0] != m.padding[1]
            or m.dilation != (1, 1) or m.groups != 1 or m.bias is None or isinstance(m.padding, str)):
        raise ValueError("LPIPS: expected square, undilated, ungrouped convolutions with a bias")
    return (m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0])


def _single(v) -> int:
    return int(v[0] if isinstance(v, (tuple, list)) else v)


def _program(net: nn.Module):
    """the network as a list of steps over named tensors, read off the module tree (so an adopted reference tree and our own
    give the same program): ("conv", src, dst, Conv2d, shape) | ("pool", src, dst) | ("tap", src, k, lin Conv2d)"""
    from neurad_studio_amd.ops_lpips import CONV_SHAPES

    steps, cur, n_conv, n_pool = [], "image", 0, 0
    for k in range(5):
        for m in list(getattr(net.net, f"slice{k + 1}").modules())[1:]:
            if isinstance(m, (nn.Sequential, nn.ReLU)):
                continue
            if isinstance(m, nn.Conv2d):
                shape = _conv_shape(m)
                if n_conv >= 5 or shape != CONV_SHAPES[n_conv]:
                    raise ValueError(f"LPIPS: convolution {n_conv + 1} is {shape}, not AlexNet's")
                n_conv += 1
                steps.append(("conv", cur, f"conv{n_conv}", m, shape))
                cur = f"conv{n_conv}"
            elif isinstance(m, nn.MaxPool2d):
                if (_single(m.kernel_size), _single(m.stride), _single(m.padding), m.ceil_mode) != (3, 2, 0, False):
                    raise ValueError("LPIPS: expected max_pool2d(3, 2) in floor mode without padding")
                n_pool += 1
                steps.append(("pool", cur, f"pool{n_pool}"))
                cur = f"pool{n_pool}"
            else:
                raise ValueError(f"LPIPS: unexpected layer {type(m).__name__}")
        lins = [m for m in getattr(net, f"lin{k}").modules() if isinstance(m, nn.Conv2d)]
        if len(lins) != 1 or lins[0].kernel_size != (1, 1) or lins[0].bias is not None or lins[0].out_channels != 1:
            raise ValueError(f"LPIPS: lin{k} is not one bias-free 1 x 1 convolution to one channel")
        steps.append(("tap", cur, k, lins[0]))
    if n_conv != 5 or n_pool != 2 or [s[0] for s in steps].count("tap") != 5:
        raise ValueError(f"LPIPS: {n_conv} convolutions and {n_pool} pools, expected 5 and 2")
    for st in steps:
        if st[0] == "tap" and st[3].in_channels != next(s[4][1] for s in steps if s[0] == "conv" and s[2] == st[1]):
            raise ValueError(f"LPIPS: lin{st[2]} does not fit its tap")
    return steps


def _f32(t: Tensor) -> Tensor:
    t = t.detach()
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


class _Packs:
    """fragment-ordered weights; rebuilt by LPIPS when a weight's storage or version moves"""

    def __init__(self, steps):
        from neurad_studio_amd import ops_lpips

        self.steps = []
        for st in steps:
            if st[0] == "conv":
                _, src, dst, m, shape = st
                self.steps.append(("conv", src, dst, ops_lpips.conv2d_pack(_f32(m.weight)), _f32(m.bias), shape))
            elif st[0] == "tap":
                self.steps.append(("tap", st[1], st[2], _f32(st[3].weight).reshape(-1)))
            else:
                self.steps.append(st)


def _nchw_pair(img1: Tensor, img2: Tensor) -> Tuple[Tensor, Tensor]:
    if img1.shape != img2.shape:
        raise ValueError(f"LPIPS: image shapes differ: {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.dim() == 3 and img1.shape[-1] == 3:
        img1, img2 = img1.permute(2, 0, 1)[None], img2.permute(2, 0, 1)[None]
    if img1.dim() != 4 or img1.shape[1] != 3 or img1.shape[0] < 1:
        raise ValueError(f"LPIPS: expected [B, 3, H, W] or [H, W, 3] images, got {tuple(img1.shape)}")
    if img1.shape[2] < MIN_SIZE or img1.shape[3] < MIN_SIZE:
        raise ValueError(f"LPIPS: images of {img1.shape[2]} x {img1.shape[3]} are smaller than {MIN_SIZE} x {MIN_SIZE}")
    return img1, img2


def out_of_range_error() -> ValueError:
    return ValueError("Expected both input arguments to be normalized tensors with shape [N, 3, H, W] and all values in the "
                      "[0,1] range (normalize=True); a value is outside [0, 1] or not finite.")


class LPIPS(nn.Module):
    """``value = m(img1, img2)``: a 0-dim tensor on the inputs' device, the batch mean.  ``pairs`` returns the per-pair values
    and the device flag of the value-range check (``None`` on a CPU path, which checks at once)."""

    def __init__(self, net: Optional[nn.Module] = None, eps_mode: int = EPS_INSIDE, eps: Optional[float] = None):
        super().__init__()
        if eps_mode not in DEFAULT_EPS:
            raise ValueError(f"LPIPS: eps_mode {eps_mode} not in {{EPS_INSIDE, EPS_OUTSIDE}}")
        self.net = (LpipsNet() if net is None else net).eval()
        self.net.requires_grad_(False)
        self.eps_mode, self.eps = eps_mode, float(DEFAULT_EPS[eps_mode] if eps is None else eps)
        self._steps = None
        self._packs: Optional[_Packs] = None
        self._packs_key: Optional[Tuple] = None

    @classmethod
    def from_reference(cls, module: nn.Module, **kwargs) -> "LPIPS":
        """adopt a torchmetrics LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True): its ``net`` tree becomes
        ours, no tensor is copied"""
        if not getattr(module, "normalize", True):
            raise ValueError("LPIPS.from_reference: the reference object takes [-1, 1] images (normalize=False)")
        return cls(net=module.net, **kwargs)

    @classmethod
    def from_torchvision(cls, **kwargs) -> "LPIPS":
        """torchvision's pretrained AlexNet features (only where torchvision is importable); the lin weights are NOT part of
        torchvision and stay as initialised: load them from an LPIPS checkpoint"""
        import torchvision

        feats = torchvision.models.alexnet(weights=torchvision.models.AlexNet_Weights.DEFAULT).features
        m = cls(**kwargs)
        with torch.no_grad():
            for name, p in m.net.net.named_parameters():  # slice{k}.{i}.{weight|bias}
                _, i, leaf = name.split(".")
                p.copy_(getattr(feats[int(i)], leaf))
        return m

    def train(self, mode: bool = True) -> "LPIPS":
        """the network is frozen and stays in eval mode, as torchmetrics keeps its own"""
        super().train(mode)
        self.net.eval()
        return self

    def steps(self):
        if self._steps is None:
            self._steps = _program(self.net)
        return self._steps

    def cache_key(self) -> Tuple:
        key = []
        for st in self.steps():
            if st[0] == "conv":
                m = st[3]
                key.append((m.weight.data_ptr(), m.weight._version, m.bias.data_ptr(), m.bias._version, m.weight.dtype))
            elif st[0] == "tap":
                key.append((st[3].weight.data_ptr(), st[3].weight._version, st[3].weight.dtype))
        return tuple(key)

    def packs(self) -> _Packs:
        key = self.cache_key()
        if self._packs is None or key != self._packs_key:
            self._packs, self._packs_key = _Packs(self.steps()), key
        return self._packs

    def _pairs_device(self, a: Tensor, b: Tensor) -> Tuple[Tensor, Tensor]:
        from neurad_studio_amd import ops_lpips

        with torch.no_grad():
            sl = self.net.scaling_layer
            # [B, 3, H, W] -> NHWC; a channels_last input is already that in memory and is not copied
            x, flag = ops_lpips.stage_images(_f32(a).permute(0, 2, 3, 1).contiguous(), _f32(b).permute(0, 2, 3, 1).contiguous(),
                                             _f32(sl.shift), _f32(sl.scale))
            t, out = {"image": x}, None
            for st in self.packs().steps:
                if st[0] == "conv":
                    _, src, dst, wf, bias, shape = st
                    t[dst] = ops_lpips.conv2d(t.pop(src), wf, shape, bias=bias, relu=True)
                elif st[0] == "pool":
                    t[st[2]] = ops_lpips.maxpool3s2_fwd(t.pop(st[1]))
                else:  # (a tap runs before the layer that consumes -- and drops -- its tensor)
                    out = ops_lpips.lpips_head(t[st[1]], st[3], self.eps_mode, self.eps, out=out)
            return out, flag

    def torch_pairs(self, a: Tensor, b: Tensor) -> Tensor:
        """per-pair values of two [B, 3, H, W] batches through the module's own ``nn.Conv2d`` layers, on whatever device they
        are: what a CPU call runs, and the baseline scripts/bench_lpips.py times the kernels against"""
        x = torch.cat([a, b]).to(self.net.scaling_layer.shift.dtype)
        if bool(((x < 0) | (x > 1) | ~torch.isfinite(x)).any()):
            raise out_of_range_error()
        n = a.shape[0]
        sl = self.net.scaling_layer  # (its buffers, not its forward: an adopted tree need not have one we know)
        t, out = {"image": (2 * x - 1 - sl.shift.reshape(1, 3, 1, 1)) / sl.scale.reshape(1, 3, 1, 1)}, 0
        for st in self.steps():
            if st[0] == "conv":
                t[st[2]] = torch.relu(st[3](t[st[1]]))
            elif st[0] == "pool":
                t[st[2]] = torch.nn.functional.max_pool2d(t[st[1]], 3, 2)
            else:
                f = t[st[1]]
                s = (f * f).sum(dim=1, keepdim=True)
                nf = f / torch.sqrt(self.eps + s) if self.eps_mode == EPS_INSIDE else f / (torch.sqrt(s) + self.eps)
                out = out + st[3]((nf[:n] - nf[n:]) ** 2).mean(dim=(1, 2, 3))
        return out

    def pairs(self, img1: Tensor, img2: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        """-> (per-pair values [B], flag): on a GPU the flag is a device int32 [1], 1 when an input value is outside [0, 1] or
        not finite, and NOTHING has been read back -- whoever transfers the values takes the flag along and raises
        ``out_of_range_error()``; on other devices the check has been made and the flag is None"""
        if img1.requires_grad or img2.requires_grad:
            raise NotImplementedError("LPIPS is a metric here: no gradient (detach the inputs)")
        a, b = _nchw_pair(img1, img2)
        if a.is_cuda:
            return self._pairs_device(a, b.to(a.device))
        with torch.no_grad():
            return self.torch_pairs(a, b), None

    def forward(self, img1: Tensor, img2: Tensor) -> Tensor:
        return self.pairs(img1, img2)[0].mean()
