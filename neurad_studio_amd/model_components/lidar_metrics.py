"""Lidar scan metrics: a drop-in for the reference's ``chamfer_distance`` (utils/math.py:745-798).

On the device the point sets go to the brute-force nearest-neighbour kernel (``ops.chamfer_distance``): direct fp32
differences, float64 sums in a fixed order, one launch sequence whatever the size -- where the reference walks
``2 ceil(N / chunk_size)`` blocks of ``torch.cdist`` in its ``|a|^2 + |b|^2 - 2ab`` form.  On CPU tensors a plain torch
fallback with direct differences runs (tests, tooling); it is not a product path.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch
from torch import Tensor

from .. import ops

_CPU_ROWS = 1024  # rows of the [rows, M, 3] difference block of the CPU fallback


def nearest_sq_dist_torch(query: Tensor, target: Tensor, query_valid: Optional[Tensor] = None,
                          target_valid: Optional[Tensor] = None) -> Tensor:
    """``ops.nearest_sq_dist`` in plain torch, direct differences: +inf without a valid target, 0 for an invalid query, NaN
    distances ignored (a NaN target never wins, a NaN query stays at +inf)"""
    q, t = query[:, :3], target[:, :3]
    if target_valid is not None:
        t = t[target_valid.reshape(-1).bool()]
    out = torch.full((q.shape[0],), float("inf"), dtype=q.dtype, device=q.device)
    if t.shape[0]:
        for i in range(0, q.shape[0], _CPU_ROWS):
            d = ((q[i:i + _CPU_ROWS, None, :] - t[None, :, :]) ** 2).sum(-1)
            out[i:i + _CPU_ROWS] = torch.nan_to_num(d, nan=float("inf"), posinf=float("inf")).amin(dim=1)
    if query_valid is not None:
        out = torch.where(query_valid.reshape(-1).bool(), out, torch.zeros_like(out))
    return out


def masked_return_metrics(pred, distance, intensity, target_intensity, ray_drop_logits, did_return) -> Dict[str, Tensor]:
    """median_l2 / mean_rel_l2 / rmse over the returned rays and the ray-drop accuracy (models/neurad.py:268-270, 477-483,
    600-609) as masked reductions: pred, distance, intensity, target_intensity, ray_drop_logits [n,1], did_return [n] bool ->
    0-dim device tensors, no ``x[mask]`` (a nonzero + a device->host read each)"""
    ret = did_return[:, None]
    n_ret = ret.sum().clamp_min(1)
    sq = (pred - distance) ** 2
    # median over the returned rays: the lower of the two middle values (torch.median), via a sort with the others at
    # +inf and a device-side index
    srt = torch.where(ret, sq, torch.full_like(sq, float("inf"))).reshape(-1).sort().values
    return {
        "depth_median_l2": srt.gather(0, ((n_ret - 1) // 2).reshape(1))[0],
        "depth_mean_rel_l2": (torch.where(ret, ((pred - distance) / distance) ** 2, torch.zeros_like(sq))).sum() / n_ret,
        "intensity_rmse": (torch.where(ret, (intensity - target_intensity) ** 2, torch.zeros_like(sq)).sum() / n_ret).sqrt(),
        "ray_drop_accuracy": ((ray_drop_logits.sigmoid() > 0.5).squeeze(-1) == ~did_return).float().mean(),
    }


LIDAR_EVAL_KEYS = ("depth_median_l2", "depth_mean_rel_l2", "intensity_rmse", "ray_drop_accuracy", "chamfer_distance")
# with outputs["median_depth"] / ["median_points"] (the plugin's ``median_depth`` flag): the same metrics on the median depth
LIDAR_EVAL_MEDIAN_KEYS = ("median_depth_median_l2", "median_depth_mean_rel_l2", "median_chamfer_distance")


def scalars_to_host(values: Tensor) -> List[float]:
    """THE device->host transfer of ``lidar_eval_metrics`` (one per scan)"""
    return values.tolist()


def lidar_eval_metrics(outputs: Dict[str, Tensor], scan: Tensor, distance: Tensor, did_return: Tensor,
                       ray_drop_loss_mult: float, non_return_lidar_distance: float,
                       to_host: Callable[[Tensor], List[float]] = scalars_to_host) -> Dict[str, float]:
    """The lidar branch of NeuRADModel.get_image_metrics_and_images (models/neurad.py:596-620) for a rendered scan, on the
    device: outputs["depth" | "intensity" | "ray_drop_logits"] [n,1] and outputs["points"] [n, >= 3] (lidar frame) of the n
    rays of ``scan`` [n, >= 4] (xyz, intensity, ...), distance [n,1], did_return [n] bool.  Masked reductions instead of
    boolean indexing; the chamfer distance on the masked point sets (predicted to return -> returned, normalised by the
    returned count); the reference's fallback -- the mean range of the returned points where no ray is predicted to return
    or none returned -- chosen with ``torch.where``; the five scalars stacked and read with ONE transfer (``to_host``).
    Every value is a Python float: the reference returns a 0-dim tensor for ``chamfer_distance`` in its fallback case.
    With outputs["median_depth"] [n,1] and outputs["median_points"] the dict also carries LIDAR_EVAL_MEDIAN_KEYS, from the
    same code on those two, and the one transfer reads eight scalars."""
    depth, logits = outputs["depth"], outputs["ray_drop_logits"]
    m = masked_return_metrics(depth, distance, outputs["intensity"], scan[:, 3:4], logits, did_return)
    # the accuracy is a ratio of two integers: through float64, so that the fp32 result is the correctly rounded quotient the
    # reference's CPU mean gives (the device's fp32 mean multiplies by a rounded 1 / n and can land one ulp off)
    m["ray_drop_accuracy"] = ((logits.sigmoid() > 0.5).squeeze(-1) == ~did_return).double().mean()
    if ray_drop_loss_mult > 0.0:  # models/neurad.py:610-613
        pred_return = (logits.sigmoid() < 0.5).squeeze(-1)
    else:
        pred_return = (depth < non_return_lidar_distance).squeeze(-1)
    fallback = torch.where(did_return, scan[:, :3].norm(dim=-1), scan.new_zeros(())).sum() / did_return.sum()

    def chamfer_of(points: Tensor, pred_return: Tensor) -> Tensor:
        chamfer = ops.chamfer_distance(points.float(), scan.float(), source_valid=pred_return, target_valid=did_return,
                                       normalize_with_target=True)
        return torch.where(pred_return.any() & did_return.any(), chamfer, fallback.float())

    m["chamfer_distance"] = chamfer_of(outputs["points"], pred_return)
    keys = LIDAR_EVAL_KEYS
    if "median_depth" in outputs and "median_points" in outputs:
        # the same code on the median depth and its points (SplatAD's names, models/splatad.py:1345-1346,1505); where the
        # returns are predicted by distance, by the median depth's own
        median = outputs["median_depth"]
        mm = masked_return_metrics(median, distance, outputs["intensity"], scan[:, 3:4], logits, did_return)
        m["median_depth_median_l2"], m["median_depth_mean_rel_l2"] = mm["depth_median_l2"], mm["depth_mean_rel_l2"]
        if not ray_drop_loss_mult > 0.0:
            pred_return = (median < non_return_lidar_distance).squeeze(-1)
        m["median_chamfer_distance"] = chamfer_of(outputs["median_points"], pred_return)
        keys = LIDAR_EVAL_KEYS + LIDAR_EVAL_MEDIAN_KEYS
    return dict(zip(keys, to_host(torch.stack([m[k].float().reshape(()) for k in keys]))))


def chamfer_distance(source_pc: Tensor, target_pc: Tensor, chunk_size: Optional[int] = None,
                     normalize_with_target: bool = False) -> Tensor:
    """The reference's signature.  ``chunk_size`` is accepted and ignored: nothing here is sized by it.  -> 0-dim tensor
    (fp32 on the device)."""
    del chunk_size
    source_pc, target_pc = source_pc.reshape(-1, source_pc.shape[-1]), target_pc.reshape(-1, target_pc.shape[-1])
    if source_pc.is_cuda:
        return ops.chamfer_distance(source_pc.float(), target_pc.float(), normalize_with_target=normalize_with_target)
    s2t = nearest_sq_dist_torch(source_pc, target_pc).double().sum()
    t2s = nearest_sq_dist_torch(target_pc, source_pc).double().sum()
    total = s2t + t2s
    if normalize_with_target:
        total = total / target_pc.shape[0]
    return total.to(source_pc.dtype)
