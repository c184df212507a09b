"""Losses that consume the sampler outputs every training step (mirror of the two functions NeuRADModel calls,
nerfstudio/model_components/losses.py:107-112,137-156,645-705; call sites models/neurad.py:262,524,541-545).

Same signatures: ``(weights_list, ray_samples_list) -> scalar``.  One wavefront per ray and per proposal level instead
of ~40 torch kernels; gradients reach what the reference's autograd reaches (the proposal weights for the interlevel
loss -- the fine histogram is detached there --, the final weights for the distortion loss)."""
from __future__ import annotations

from typing import List, Sequence

import torch
from torch import Tensor

from .. import autograd as ag
from ..cameras.rays import RaySamples

PULSE_WIDTHS = (0.03, 0.003)  # losses.py:677


def ray_samples_to_sdist(ray_samples: RaySamples) -> Tensor:
    """spacing-space bin edges [R, S+1] (losses.py:107-112)"""
    sdist = getattr(ray_samples, "sdist", None)
    if sdist is not None:  # the fused training path carries the edges as one tensor
        return sdist
    return torch.cat([ray_samples.spacing_starts[..., 0], ray_samples.spacing_ends[..., -1:, 0]], dim=-1)


def zipnerf_interlevel_loss(weights_list: Sequence[Tensor], ray_samples_list: List[RaySamples]) -> Tensor:
    c = ray_samples_to_sdist(ray_samples_list[-1]).detach()
    w = weights_list[-1].squeeze(-1).detach()
    loss = None
    for i, (ray_samples, weights) in enumerate(zip(ray_samples_list[:-1], weights_list[:-1])):
        term = ag.InterlevelLossFn.apply(c, w, ray_samples_to_sdist(ray_samples).detach(), weights.squeeze(-1), PULSE_WIDTHS[i])
        loss = term if loss is None else loss + term
    return c.new_zeros(()) if loss is None else loss


def distortion_loss(weights_list: Sequence[Tensor], ray_samples_list: List[RaySamples]) -> Tensor:
    return ag.DistortionLossFn.apply(ray_samples_to_sdist(ray_samples_list[-1]).detach(), weights_list[-1].squeeze(-1))


def packed_addressing(segments, ray_indices, num_rays) -> Tensor:
    """segments int64 [R+1] from exactly one of the two addressings of packed samples: ``segments`` itself, or the sorted
    ``ray_indices`` [M] with ``num_rays`` (derived on the device, no host read)"""
    if (segments is None) == (ray_indices is None):
        raise ValueError("packed samples are addressed by exactly one of segments= and ray_indices= (with num_rays=)")
    if segments is not None:
        if num_rays is not None and int(num_rays) != segments.shape[0] - 1:
            raise ValueError(f"segments holds {segments.shape[0] - 1} rays, num_rays says {int(num_rays)}")
        return segments
    if num_rays is None:
        raise ValueError("ray_indices= needs num_rays=")
    return ag.ops.packed_segments(ray_indices, int(num_rays))


def packed_distortion_loss(weights: Tensor, starts: Tensor, ends: Tensor, *, segments=None, ray_indices=None,
                           num_rays=None) -> Tensor:
    """The distortion loss (losses.py:137-156; nerfstudio_distortion_loss, losses.py:159-200) on packed,
    occupancy-marched samples: the mean over ALL rays of
        sum_i sum_j w_i w_j |m_i - m_j| + sum_i w_i^2 (end_i - start_i) / 3,      m_i = (start_i + end_i) / 2,
    in O(n) per ray and float64 (csrc/losses.hip; the contract and its error bound: include/neurad_hip.h at
    nrhip_packed_distortion_loss).  A ray without samples contributes 0.  weights [M] or [M,1] (what
    ``VolumetricSampler.render_train`` returns); starts / ends [M] or [M,1] with midpoints non-decreasing within a ray;
    exactly one of ``segments`` int64 [R+1] and ``ray_indices`` int64 [M] + ``num_rays``.  Gradient: to the weights only.

    The caller chooses the metric of ``starts`` / ``ends``.  The march's Euclidean ``t_starts`` / ``t_ends`` work as they
    are; for an unbounded scene one wants the reference's normalised spacing instead, a monotone map that keeps the order::

        sp = PowerSpacing(nears[ray_indices], fars[ray_indices], lam, scaling)
        loss = packed_distortion_loss(out["weights"], sp.to_spacing(out["t_starts"]), sp.to_spacing(out["t_ends"]),
                                      ray_indices=out["ray_indices"], num_rays=R)
    """
    seg = packed_addressing(segments, ray_indices, num_rays)
    return ag.PackedDistortionLossFn.apply(starts.detach().reshape(-1), ends.detach().reshape(-1), weights.reshape(-1), seg)
