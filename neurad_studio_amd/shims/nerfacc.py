"""nerfacc-shaped module on HIP kernels: the three functions neurad-studio calls
(models/neurad.py:716-723,734; model_components/renderers.py:88,130,133,345,404,407,455,486), dense and -- with
``ray_indices`` + ``n_rays`` or ``packed_info`` -- packed (csrc/packed_composite.h), and ``pack_info``.
Put this directory on sys.path as ``nerfacc`` or import it directly."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import autograd as ag


def _segments(packed_info, ray_indices, n_rays, prefix_trans=None) -> Tensor:
    """segments int64 [R+1] of a packed call: from packed_info [R,2] (start, count) or sorted ray_indices + n_rays"""
    if prefix_trans is not None:
        raise NotImplementedError("prefix_trans")
    if packed_info is not None:
        info = packed_info.to(torch.int64)
        seg = torch.empty((info.shape[0] + 1,), dtype=torch.int64, device=info.device)
        seg[:-1] = info[:, 0]
        seg[-1:] = (info[-1:, 0] + info[-1:, 1]) if info.shape[0] else 0
        return seg
    if n_rays is None:
        raise ValueError("packed mode: ray_indices needs n_rays")
    return ag.ops.packed_segments(ray_indices, int(n_rays))


def pack_info(ray_indices: Tensor, n_rays: Optional[int] = None) -> Tensor:
    """nerfacc.pack_info: sorted ray_indices [M] -> packed_info [n_rays, 2] (start, count) per ray"""
    if n_rays is None:
        raise ValueError("pack_info: n_rays is needed (no host synchronisation to find it)")
    seg = ag.ops.packed_segments(ray_indices, int(n_rays))
    return torch.stack([seg[:-1], seg[1:] - seg[:-1]], -1)


def render_weight_from_alpha(alphas: Tensor, packed_info=None, ray_indices=None, n_rays=None,
                             prefix_trans=None) -> Tuple[Tensor, Tensor]:
    if packed_info is not None or ray_indices is not None:
        return ag.PackedWeightFromAlphaFn.apply(alphas, _segments(packed_info, ray_indices, n_rays, prefix_trans))
    return ag.WeightFromAlphaFn.apply(alphas.contiguous())


def render_weight_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info=None, ray_indices=None,
                               n_rays=None, prefix_trans=None) -> Tuple[Tensor, Tensor, Tensor]:
    if packed_info is not None or ray_indices is not None:
        return ag.PackedWeightFromDensityFn.apply(t_starts, t_ends, sigmas,
                                                  _segments(packed_info, ray_indices, n_rays, prefix_trans))
    return ag.WeightFromDensityFn.apply(t_starts.contiguous(), t_ends.contiguous(), sigmas.contiguous())


def accumulate_along_rays(weights: Tensor, values: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                          n_rays: Optional[int] = None) -> Tensor:
    if ray_indices is not None:
        return ag.PackedAccumulateFn.apply(weights, values, _segments(None, ray_indices, n_rays))
    if values is None:
        return weights.sum(-1, keepdim=True) if weights.requires_grad else ag.ops.accumulate_along_rays(weights.contiguous())
    return ag.AccumulateFn.apply(weights.contiguous(), values.contiguous())


class OccGridEstimator(torch.nn.Module):
    """nerfacc.OccGridEstimator-shaped module: a multi-level occupancy grid with ``sampling`` as VolumetricSampler calls it
    (model_components/ray_samplers.py:527-540), ``update_every_n_steps`` and ``mark_invisible_cells``.  Marching rule:
    csrc/occgrid.hip; update rule: csrc/occgrid_update.h (modelled on nerfacc 0.5, parity with nerfacc itself unpinned --
    its own ``state_dict`` is not loadable here).

    Buffers: ``aabbs`` [L,6] (level l: the level-0 box scaled by 2^l about its centre), ``occs`` fp32 [L*res^3],
    ``binaries`` bool [L,res,res,res], ``resolution`` int32 [3] and ``fresh``.  A fresh estimator has every binary set and
    every occ one -- "nothing known, march everything"; the first update or ``mark_invisible_cells`` ends that state by
    zeroing ``occs`` first, so the EMA starts from zero.  ``binaries`` may be edited in place."""

    def __init__(self, roi_aabb, resolution: int = 128, levels: int = 1, device="cuda"):
        super().__init__()
        from .. import ops

        if levels < 1:
            raise ValueError("levels must be >= 1")
        boxes = ops.occgrid_level_aabbs(roi_aabb, levels)
        self.levels, self.cells_per_lvl = int(levels), int(resolution) ** 3
        self.register_buffer("aabbs", boxes.to(device))
        self.register_buffer("binaries", torch.ones((levels, resolution, resolution, resolution), dtype=torch.bool,
                                                    device=device))
        self.register_buffer("occs", torch.ones((levels * self.cells_per_lvl,), dtype=torch.float32, device=device))
        self.register_buffer("resolution", torch.tensor([resolution] * 3, dtype=torch.int32))
        self.register_buffer("fresh", torch.ones((), dtype=torch.bool))
        # host mirrors: the march and the update read the boxes and the flag without a device read
        self._aabbs_host, self._fresh_host, self._scratch = boxes.clone(), True, None

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._aabbs_host = self._fresh_host = None  # re-read once, at the next use

    def _spec(self):
        from .. import ops

        if self._aabbs_host is None:
            self._aabbs_host = self.aabbs.detach().cpu().clone()
        return ops.OccGridSpec(self._aabbs_host, self.binaries)

    def _end_fresh(self) -> None:
        if self._fresh_host is None:
            self._fresh_host = bool(self.fresh.item())
        if self._fresh_host:
            self.occs.zero_()
            self.fresh.fill_(False)
            self._fresh_host = False

    def _get_scratch(self) -> dict:
        from .. import ops

        sc = self._scratch
        if sc is None or sc["workspace"].device != self.occs.device:
            sc = self._scratch = ops.occgrid_update_scratch(self.levels, self.binaries.shape[-1], self.occs.device)
        return sc

    @torch.no_grad()
    def update_every_n_steps(self, step: int, occ_eval_fn, occ_thre: float = 1e-2, ema_decay: float = 0.95,
                             warmup_steps: int = 256, n: int = 16) -> None:
        """nerfacc's training-loop call: every ``n`` steps, evaluate ``occ_eval_fn`` ([N,3] positions -> [N,1] or [N]
        density x step size) at the candidate cells and fold it into the grid.  Training mode only."""
        if not self.training:
            raise RuntimeError("You should only call this function only during training. Please call _update() directly "
                               "if you want to update the field during inference.")
        if step % n == 0:
            self._update(step=step, occ_eval_fn=occ_eval_fn, occ_thre=occ_thre, ema_decay=ema_decay,
                         warmup_steps=warmup_steps)

    @torch.no_grad()
    def _update(self, step: int, occ_eval_fn, occ_thre: float = 1e-2, ema_decay: float = 0.95, warmup_steps: int = 256,
                cell_draws=None, sel_draws=None, jitter=None):
        """One update (csrc/occgrid_update.h).  The three draw tensors are injected by tests; by default they are made on
        the device.  From the second call on: no host synchronisation, no allocation sized by data.
        -> (cell_ids, counts, positions) of the candidates, views of the cached scratch."""
        from .. import ops

        self._end_fresh()
        return ops.occgrid_update(self._spec(), self.occs, occ_eval_fn, step, occ_thre, ema_decay, warmup_steps,
                                  cell_draws=cell_draws, sel_draws=sel_draws, jitter=jitter, scratch=self._get_scratch())

    @torch.no_grad()
    def mark_invisible_cells(self, K, c2w, width: int, height: int, near_plane: float = 0.0) -> None:
        """Cells no camera sees -- or one sees closer than ``near_plane`` -- get occs = -1 and are never evaluated or
        occupied again; the others get occs = 0.  K [N,3,3] or [1,3,3], c2w [N,3,4] or [N,4,4] (OpenCV)."""
        from .. import ops

        self._end_fresh()
        dev = self.occs.device
        ops.occgrid_mark_invisible(self._spec(), self.occs, K.to(dev, torch.float32), c2w.to(dev, torch.float32), width,
                                   height, near_plane)

    def sampling(self, rays_o, rays_d, sigma_fn=None, alpha_fn=None, near_plane: float = 0.0, far_plane: float = 1e10,
                 t_min=None, t_max=None, render_step_size: float = 1e-3, early_stop_eps: float = 1e-4,
                 alpha_thre: float = 0.0, stratified: bool = False, cone_angle: float = 0.0, actor_boxes=None):
        """actor_boxes (a keyword beyond nerfacc's signature): None = the plain march; (ops.ActorSpec, cand) = the box-aware
        march -- an interval inside the box of one of the ray's candidate actors is kept whatever its cell says
        (ops.occgrid_march).  The visibility filter below applies to whatever sigma_fn / alpha_fn return, as before."""
        from .. import ops

        t_rand = torch.rand((rays_o.shape[0],), device=rays_o.device) if stratified else None
        ri, ts, te, seg = ops.occgrid_march(self._spec(), rays_o, rays_d, render_step_size, near_plane, far_plane, t_min,
                                            t_max, cone_angle, t_rand, actor_boxes=actor_boxes)
        if (alpha_thre > 0.0 or early_stop_eps > 0.0) and (sigma_fn is not None or alpha_fn is not None) and ri.numel():
            if alpha_thre > 0.0:  # (the one host read of this route: out of scope to move it to the device)
                alpha_thre = min(alpha_thre, float(self.occs.mean().item()))
            if sigma_fn is not None:
                alphas = 1.0 - torch.exp(-sigma_fn(ts, te, ri) * (te - ts))
            else:
                alphas = alpha_fn(ts, te, ri)
            keep = ops.packed_visibility_from_alpha(alphas.float().contiguous(), seg, early_stop_eps, alpha_thre)
            ri, ts, te = ri[keep], ts[keep], te[keep]
        return ri, ts, te
