"""Renderers with the reference's signatures (model_components/renderers.py:59-90,322-350,353-418) and
render_depth_simple (models/neurad.py:727-734) on the HIP compositing kernels: dense, and -- with ``ray_indices`` and
``num_rays`` -- over the packed samples of VolumetricSampler; ``render_packed`` is the fused packed form."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from ..cameras.rays import RaySamples
from ..shims import nerfacc


class FeatureRenderer(nn.Module):
    def forward(self, features: Tensor, weights: Tensor, ray_indices=None, num_rays=None) -> Tensor:
        return nerfacc.accumulate_along_rays(weights[..., 0], values=features, ray_indices=ray_indices, n_rays=num_rays)


class AccumulationRenderer(nn.Module):
    @classmethod
    def forward(cls, weights: Tensor, ray_indices=None, num_rays=None) -> Tensor:
        return nerfacc.accumulate_along_rays(weights[..., 0], values=None, ray_indices=ray_indices, n_rays=num_rays)


def render_depth_simple(weights: Tensor, ray_samples: RaySamples, ray_indices=None, num_rays=None) -> Tensor:
    steps = (ray_samples.frustums.starts + ray_samples.frustums.ends) / 2
    return nerfacc.accumulate_along_rays(weights[..., 0], values=steps, ray_indices=ray_indices, n_rays=num_rays)


def median_depth(weights: Tensor, starts: Tensor, ends: Tensor, ray_indices=None, num_rays=None,
                 quantile: float = 0.5) -> Tensor:
    """Median depth [R,1] (csrc/median_depth.hip; the contract: include/neurad_hip.h at nrhip_median_depth): the midpoint of
    the first sample at which the accumulated weight reaches ``quantile``.  weights / starts / ends: [R,S] or [R,S,1] dense,
    [M] or [M,1] with ``ray_indices`` and ``num_rays`` packed.  The result carries no gradient -- it is piecewise constant in
    the weights; its only dependence on the interval ends, through the crossing sample's midpoint, is not implemented and
    asking for it raises."""
    from .. import ops

    if torch.is_grad_enabled() and (starts.requires_grad or ends.requires_grad):
        raise NotImplementedError("median depth has no gradient: it is piecewise constant in the weights, and the gradient "
                                  "to starts / ends through the crossing sample's midpoint is not implemented")
    weights, starts, ends = weights.detach(), starts.detach(), ends.detach()
    if ray_indices is not None and num_rays is not None:  # packed samples of the volumetric sampler
        seg = ops.packed_segments(ray_indices, int(num_rays))
        return ops.median_depth_packed(weights.reshape(-1), starts.reshape(-1), ends.reshape(-1), seg, (quantile,))
    if weights.dim() == 3:
        weights, starts, ends = weights[..., 0], starts[..., 0], ends[..., 0]
    return ops.median_depth(weights, starts, ends, (quantile,))


class DepthRenderer(nn.Module):
    """``method="expected"`` (the default here: what NeuRAD uses, models/neurad.py:252) or ``"median"`` (the reference's own
    default, renderers.py:364): dense, and -- unlike the reference's -- packed as well.  ``quantile`` moves the median's
    threshold off one half."""

    def __init__(self, method: str = "expected", quantile: float = 0.5) -> None:
        super().__init__()
        if method not in ("expected", "median"):
            raise NotImplementedError(f"Method {method} not implemented")
        self.method, self.quantile = method, float(quantile)

    def forward(self, weights: Tensor, ray_samples: RaySamples, ray_indices=None, num_rays=None) -> Tensor:
        if self.method == "median":
            fr = ray_samples.frustums
            return median_depth(weights, fr.starts, fr.ends, ray_indices, num_rays, self.quantile)
        eps = 1e-10
        steps = (ray_samples.frustums.starts + ray_samples.frustums.ends) / 2
        if ray_indices is not None and num_rays is not None:  # packed samples of the volumetric sampler
            depth = nerfacc.accumulate_along_rays(weights[..., 0], values=steps, ray_indices=ray_indices, n_rays=num_rays)
            acc = nerfacc.accumulate_along_rays(weights[..., 0], values=None, ray_indices=ray_indices, n_rays=num_rays)
        else:
            depth = nerfacc.accumulate_along_rays(weights[..., 0], values=steps)
            acc = nerfacc.accumulate_along_rays(weights[..., 0], values=None)
        depth = depth / (acc + eps)
        return torch.clip(depth, steps.min(), steps.max())


class NormalsRenderer(nn.Module):
    """Weighted sum of the per-sample normals, optionally renormalised (model_components/renderers.py:462-489; the
    normalisation is safe_normalize, utils/math.py:455-468: v / (|v| + 1e-10))."""

    @classmethod
    def forward(cls, normals: Tensor, weights: Tensor, normalize: bool = True, ray_indices=None, num_rays=None) -> Tensor:
        n = nerfacc.accumulate_along_rays(weights[..., 0], values=normals, ray_indices=ray_indices, n_rays=num_rays)
        if normalize:
            n = n / (torch.linalg.norm(n, dim=-1, keepdim=True) + 1e-10)
        return n


def render_packed(features: Tensor, ray_samples: RaySamples, ray_indices: Tensor, num_rays: int, *,
                  density: Optional[Tensor] = None, alpha: Optional[Tensor] = None, median_depth: bool = False) -> dict:
    """Fused compositing of the packed samples ``VolumetricSampler.forward`` returns: features [M,C] and exactly one of
    density / alpha ([M] or [M,1]) -> ``features`` [R,C], ``depth`` [R,1] (render_depth_simple: sum w mid, not normalised),
    ``accumulation`` [R,1] and the per-sample ``weights`` [M,1], one kernel forward and one backward.  ``median_depth``:
    also ``median_depth`` [R,1] from those weights (one more launch; no gradient, an empty ray gets 0)."""
    from .. import autograd as ag

    if (density is None) == (alpha is None):
        raise ValueError("render_packed: give exactly one of density / alpha")
    x = density if density is not None else alpha
    seg = ag.ops.packed_segments(ray_indices, int(num_rays))
    f, d, a, w = ag.PackedCompositeFn.apply(ray_samples.frustums.starts.reshape(-1), ray_samples.frustums.ends.reshape(-1),
                                            x.reshape(-1), features, seg, density is not None)
    out = {"features": f, "depth": d, "accumulation": a, "weights": w[..., None]}
    if median_depth:
        fr = ray_samples.frustums
        out["median_depth"] = ag.ops.median_depth_packed(w.detach(), fr.starts.detach().reshape(-1),
                                                         fr.ends.detach().reshape(-1), seg)
    return out
