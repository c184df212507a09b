"""Camera image metrics: PSNR and SSIM of a rendered image against its ground truth, drop-ins for the two torchmetrics objects
of the reference (``self.psnr = PeakSignalNoiseRatio(data_range=1.0)``, ``self.ssim = structural_similarity_index_measure``,
models/neurad.py:265-266, called at 465 and 585-586).

On the device both come from ONE launch sequence of csrc/image_eval.hip (``ops.image_metrics``: the squared error and the data
range in a first pass, the windowed moments of shifted values in a second, float64 sums in a fixed order) and travel to the
host in ONE transfer, where the reference pays a ``float()`` per metric and forms each variance as E[x^2] - mu^2 in fp32.  On
CPU tensors a plain torch float64 fallback runs (tests, tooling); it is not a product path.

LPIPS, the third metric of that method, is model_components/lpips.py (csrc/lpips.hip).  ``image_eval_metrics3`` and
``ImageEvalTriple`` add it to the same ONE transfer, which also carries the device flag of torchmetrics' value-range check;
``image_eval_metrics`` and ``ImageEvalPair`` are unchanged and leave LPIPS to the caller.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from .. import ops

IMAGE_EVAL_KEYS = ("psnr", "ssim")
IMAGE_EVAL_KEYS3 = ("psnr", "ssim", "lpips")
WINDOW, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def gaussian_window(dtype=torch.float64, device=None) -> Tensor:
    """the 11 taps exp(-(d / 1.5)^2 / 2), d = -5..5, normalised to sum 1"""
    d = torch.arange(WINDOW, dtype=dtype, device=device) - (WINDOW - 1) / 2
    g = torch.exp(-((d / SIGMA) ** 2) / 2)
    return g / g.sum()


def _hwc(t: Tensor) -> Tensor:
    """[H,W,C] or [1,C,H,W] -> [H,W,C] (a view)"""
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError(f"one image per call, got a batch of {t.shape[0]}")
        t = t[0].permute(1, 2, 0)
    if t.dim() != 3:
        raise ValueError(f"expected [H,W,C] or [1,C,H,W], got {tuple(t.shape)}")
    return t


def image_psnr_torch(a: Tensor, b: Tensor, psnr_range: float = 1.0) -> Tensor:
    """``ops.image_psnr`` in plain torch, float64 -> 0-dim float64 tensor (+inf for identical images)"""
    mse = ((a.detach().double() - b.detach().double()) ** 2).mean()
    return 10.0 * torch.log10(float(psnr_range) ** 2 / mse)


def image_metrics_torch(a: Tensor, b: Tensor, psnr_range: float = 1.0, return_map: bool = False):
    """``ops.image_metrics`` in plain torch, float64, every window that lies inside the image (what torchmetrics' reflect pad
    and crop leave) -> (psnr, ssim[, map [H-10, W-10, C]]) as float64 tensors"""
    a, b = _hwc(a).detach().double(), _hwc(b).detach().double()
    if a.shape != b.shape:
        raise ValueError(f"image shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
    h, w, c = a.shape
    if h < WINDOW or w < WINDOW:
        raise ValueError(f"image {h} x {w} is smaller than the {WINDOW} x {WINDOW} SSIM window")
    r = torch.maximum(a.max() - a.min(), b.max() - b.min())
    c1, c2 = (K1 * r) ** 2, (K2 * r) ** 2
    g = gaussian_window(device=a.device)
    win = (g[:, None] * g[None, :]).expand(c, 1, WINDOW, WINDOW).contiguous()
    x = torch.stack([a, b, a * a, b * b, a * b]).permute(0, 3, 1, 2)  # [5, C, H, W]
    mu_a, mu_b, e_aa, e_bb, e_ab = torch.nn.functional.conv2d(x, win, groups=c)
    var_a, var_b, cov = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    s = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    s = s.permute(1, 2, 0)
    psnr, ssim = image_psnr_torch(a, b, psnr_range), s.mean()
    return (psnr, ssim, s) if return_map else (psnr, ssim)


def scalars_to_host(values: Tensor) -> List[float]:
    """THE device->host transfer of ``image_eval_metrics`` (one per image)"""
    return values.tolist()


def image_eval_metrics(rgb: Tensor, image: Tensor,
                       to_host: Callable[[Tensor], List[float]] = scalars_to_host) -> Dict[str, float]:
    """psnr and ssim of a rendered image ``rgb`` against ``image`` ([H,W,C] or the reference's [1,C,H,W] views, H, W >= 11;
    ValueError below that, where the reference's reflect pad fails as well) -> {"psnr": float, "ssim": float}, both scalars
    in ONE transfer (``to_host``)."""
    if rgb.is_cuda:
        psnr, ssim = ops.image_metrics(rgb, image.to(rgb.device))
    else:
        psnr, ssim = image_metrics_torch(rgb, image)
    return dict(zip(IMAGE_EVAL_KEYS, to_host(torch.stack([psnr, ssim]))))


def _lpips_scalars(lpips, preds: Tensor, target: Tensor) -> List[Tensor]:
    """-> [value, flag] as 0-dim tensors of one dtype on the images' device (flag 0 where the check has been made already)"""
    values, flag = lpips.pairs(preds, target)
    value = values.mean()
    return [value, torch.zeros_like(value) if flag is None else flag[0].to(value.dtype)]


def _raise_if_flagged(flag: float) -> None:
    if flag != 0.0:
        from .lpips import out_of_range_error

        raise out_of_range_error()


def image_eval_metrics3(rgb: Tensor, image: Tensor, lpips,
                        to_host: Callable[[Tensor], List[float]] = scalars_to_host) -> Dict[str, float]:
    """``image_eval_metrics`` plus LPIPS (``lpips``: a model_components.lpips.LPIPS) -> {"psnr", "ssim", "lpips"}: floats from
    ONE transfer of four scalars.  The fourth is the flag of LPIPS' value-range check (torchmetrics' _valid_img, a host read of
    its own there): when it is set, the ValueError torchmetrics would have raised is raised here, after the read."""
    if rgb.is_cuda:
        psnr, ssim = ops.image_metrics(rgb, image.to(rgb.device))
    else:
        psnr, ssim = image_metrics_torch(rgb, image)
    value, flag = _lpips_scalars(lpips, rgb, image.to(rgb.device))
    dtype = torch.promote_types(psnr.dtype, value.dtype)  # (fp32 on the device; the float64 fallback keeps its digits)
    *values, flagged = to_host(torch.stack([v.to(dtype) for v in (psnr, ssim, value, flag)]))
    _raise_if_flagged(flagged)
    return dict(zip(IMAGE_EVAL_KEYS3, values))


def lpips_eval_metric(preds: Tensor, target: Tensor, lpips, to_host: Callable[[Tensor], List[float]] = scalars_to_host) -> float:
    """LPIPS alone, as the reference calls it (``float(self.lpips(image, rgb))``): the value and the range flag in ONE
    transfer, the ValueError after it"""
    value, flagged = to_host(torch.stack(_lpips_scalars(lpips, preds, target.to(preds.device))))
    _raise_if_flagged(flagged)
    return value


class PSNR(torch.nn.Module):
    """``PeakSignalNoiseRatio(data_range)`` as the model calls it (models/neurad.py:465): psnr(preds, target) -> 0-dim tensor
    on the tensors' device; no host read, no accumulated metric state"""

    def __init__(self, data_range: float = 1.0):
        super().__init__()
        self.data_range = float(data_range)

    def forward(self, preds: Tensor, target: Tensor) -> Tensor:
        if preds.is_cuda:
            return ops.image_psnr(preds, target.to(preds.device), self.data_range)
        return image_psnr_torch(preds, target, self.data_range).to(preds.dtype)


class ImageEvalPair:
    """``psnr`` and ``ssim`` with the reference's call shapes (``float(self.psnr(image, rgb))``, ``float(self.ssim(image,
    rgb))`` on [1,3,H,W] views, models/neurad.py:585-586) over ONE ``image_eval_metrics`` call: whichever is called first
    launches everything and does the one read; the other is served from it when it gets the same two tensors."""

    def __init__(self, to_host: Callable[[Tensor], List[float]] = scalars_to_host):
        self.to_host = to_host
        self._pair: Optional[Tuple[Tensor, Tensor]] = None
        self._values: Dict[str, float] = {}

    def _get(self, key: str, preds: Tensor, target: Tensor) -> float:
        if self._pair is None or self._pair[0] is not preds or self._pair[1] is not target:
            self._values = image_eval_metrics(preds, target, to_host=self.to_host)
            self._pair = (preds, target)
        return self._values[key]

    def psnr(self, preds: Tensor, target: Tensor) -> float:
        return self._get("psnr", preds, target)

    def ssim(self, preds: Tensor, target: Tensor) -> float:
        return self._get("ssim", preds, target)


class ImageEvalTriple:
    """``ImageEvalPair`` with ``lpips`` as the third: whichever of the three is called first on a pair of tensors launches
    everything (``image_eval_metrics3``: one transfer) and the others are served from it"""

    def __init__(self, lpips, to_host: Callable[[Tensor], List[float]] = scalars_to_host):
        self.lpips_module, self.to_host = lpips, to_host
        self._pair: Optional[Tuple[Tensor, Tensor]] = None
        self._values: Dict[str, float] = {}

    def _get(self, key: str, preds: Tensor, target: Tensor) -> float:
        if self._pair is None or self._pair[0] is not preds or self._pair[1] is not target:
            self._values = image_eval_metrics3(preds, target, self.lpips_module, to_host=self.to_host)
            self._pair = (preds, target)
        return self._values[key]

    def psnr(self, preds: Tensor, target: Tensor) -> float:
        return self._get("psnr", preds, target)

    def ssim(self, preds: Tensor, target: Tensor) -> float:
        return self._get("ssim", preds, target)

    def lpips(self, preds: Tensor, target: Tensor) -> float:
        return self._get("lpips", preds, target)


def ssim(preds: Tensor, target: Tensor) -> Tensor:
    """``structural_similarity_index_measure(preds, target)`` for one [1,C,H,W] (or [H,W,C]) pair -> 0-dim tensor on the
    tensors' device"""
    if preds.is_cuda:
        return ops.image_metrics(preds, target.to(preds.device))[1]
    return image_metrics_torch(preds, target)[1].to(preds.dtype)


def psnr(preds: Tensor, target: Tensor, data_range: float = 1.0) -> Tensor:
    """the functional form of ``PSNR``"""
    return PSNR(data_range)(preds, target)
