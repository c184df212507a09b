"""Camera pose optimisation, mode "SO3xR3": a stand-alone ``CameraOptimizer`` with the surface of the reference's module
(cameras/camera_optimizers.py:108-240 and its scaled variant, :359-379) and no nerfstudio import.

Per training step the reference gathers ``pose_adjustment[camera_indices]``, runs ``exp_map_SO3xR3`` (cameras/lie_groups.py:24-58:
about 25 small launches, six of them strided index assignments) and a ``bmm``; backwards the same ops end in an index backward
that lands every ray of a batch on a few hundred rows.  Here ``apply_to_raybundle`` on GPU tensors is ONE autograd node
(autograd.PoseApplyFn over csrc/pose_opt.hip): one launch forwards; backwards per-camera integer sums -- the same bits for any
order of the rays, no float atomics -- and the chain through the exponential map in double.  The corrected rays are fp32
whatever autocast says (the reference's ``torch.bmm`` returns fp16 under autocast: its directions are rounded through fp16), and
``[R, 3]`` also for R = 1, where the reference's ``.squeeze()`` drops the axis.  ``get_metrics_dict`` returns 0-dim device
tensors, degrees by a multiply on the device: no ``.cpu()``, where the reference synchronises twice per step.  On CPU tensors a
plain torch restatement of the same formula runs (tests, tooling); it is not a product path.

``CameraOptimizer.from_reference(module)`` adopts the reference module's Parameter object and ``weights`` buffer: optimizers,
parameter groups, state-dict names and checkpoints are untouched.  Mode "off", mode "SE3" and a module with
``non_trainable_camera_indices`` are handed back as they are.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch
from torch import Tensor, nn

CLAMP = 9.999999747378752e-05  # the fp32 value of 1e-4: what torch.clamp(nrms, 1e-4) compares an fp32 tensor with
METRIC_KEYS = ("camera_opt_translation_max", "camera_opt_translation_mean", "camera_opt_rotation_mean",
               "camera_opt_rotation_max")


@dataclass
class CameraOptimizerConfig:
    """the fields of the reference's CameraOptimizerConfig / ScaledCameraOptimizerConfig that the module reads"""

    mode: str = "SO3xR3"
    trans_l2_penalty: Union[Tuple[float, float, float], float] = 1e-2
    """plain module: a factor on the mean L2 norm of the translations; scaled module: per-axis factors on their absolute values"""
    rot_l2_penalty: float = 1e-3
    weights: Optional[Tuple[float, float, float, float, float, float]] = None
    """not None: the scaled variant -- the parameter times these weights is the tangent vector (translation first, as the
    reference's code applies them)"""


def exp_map_so3xr3(tangent: Tensor) -> Tensor:
    """[n, 6] (translation, then the so(3) tangent vector w) -> [n, 3, 4] = [R | t]:
    nrms = |w|^2, theta = sqrt(max(nrms, 1e-4)), R = sin(theta) / theta K + (1 - cos(theta)) / theta^2 K^2 + I, K v = w x v.
    Any dtype, differentiable; below the clamp the two factors are constants."""
    w = tangent[:, 3:]
    x, y, z = w.unbind(-1)
    nrms = (w * w).sum(1)
    theta = torch.clamp(nrms, CLAMP).sqrt()
    inv = 1.0 / theta
    f1 = inv * theta.sin()
    f2 = inv * inv * (1.0 - theta.cos())
    zero = torch.zeros_like(x)
    skew = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(-1, 3, 3)
    rot = f1[:, None, None] * skew + f2[:, None, None] * torch.bmm(skew, skew) + torch.eye(3, dtype=w.dtype, device=w.device)
    return torch.cat([rot, tangent[:, :3, None]], -1)


class CameraOptimizer(nn.Module):
    """parameter ``pose_adjustment`` [num_cameras, 6]; buffer ``weights`` [6] in the scaled variant (persistent, as in the
    reference: state-dict names ``pose_adjustment`` / ``weights``)"""

    def __init__(self, config, num_cameras: int, device: Union[torch.device, str] = "cpu",
                 pose_adjustment: Optional[nn.Parameter] = None, weights: Optional[Tensor] = None, **kwargs) -> None:
        super().__init__()
        if config.mode not in ("off", "SO3xR3"):
            raise NotImplementedError(f"camera optimizer mode {config.mode!r}: only 'off' and 'SO3xR3' are restated here")
        self.config = config
        self.num_cameras = num_cameras
        self.device = device
        self.non_trainable_camera_indices = None
        if pose_adjustment is not None:  # an adopted parameter: the penalties live where it lives
            device = pose_adjustment.device
        if weights is None and getattr(config, "weights", None) is not None:
            weights = torch.tensor(config.weights, dtype=torch.float32, device=device)
        self.scaled = weights is not None
        if config.mode == "SO3xR3":
            self.pose_adjustment = pose_adjustment if pose_adjustment is not None else nn.Parameter(
                torch.zeros((num_cameras, 6), device=device))
        self.register_buffer("weights", weights)
        if self.scaled:  # travels with the module, stays out of the state dict (the reference: a plain tensor attribute)
            self.register_buffer("_trans_penalty", torch.tensor(config.trans_l2_penalty, dtype=torch.float32, device=device)
                                 .expand(3).contiguous(), persistent=False)

    @classmethod
    def from_reference(cls, module):
        """the reference's CameraOptimizer / ScaledCameraOptimizer -> this class around the SAME Parameter object and
        ``weights`` buffer and the module's own config; the module itself where this class does not restate it"""
        if isinstance(module, cls):
            return module
        if module.config.mode != "SO3xR3" or getattr(module, "non_trainable_camera_indices", None) is not None:
            return module
        return cls(module.config, module.num_cameras, module.device, pose_adjustment=module.pose_adjustment,
                   weights=module._buffers.get("weights"))

    def _get_pose_adjustment(self) -> Tensor:
        return self.pose_adjustment * self.weights if self.scaled else self.pose_adjustment

    def forward(self, indices: Tensor) -> Tensor:
        """-> [n, 3, 4] corrections of the cameras ``indices`` (identity for mode "off")"""
        if self.config.mode == "off":
            return torch.eye(4, device=self.device)[None, :3, :4].tile(indices.shape[0], 1, 1)
        return exp_map_so3xr3(self._get_pose_adjustment()[indices, :])

    def apply_to_raybundle(self, raybundle) -> None:
        if self.config.mode == "off":
            return
        o, d = raybundle.origins, raybundle.directions
        idx = raybundle.camera_indices.reshape(-1)
        if o.is_cuda:
            from ..autograd import PoseApplyFn

            o2, d2 = PoseApplyFn.apply(self.pose_adjustment, self.weights, idx, o.reshape(-1, 3).float(),
                                       d.reshape(-1, 3).float())
        else:
            m = self(idx)
            o2 = o.reshape(-1, 3) + m[:, :3, 3]
            d2 = torch.bmm(m[:, :3, :3], d.reshape(-1, 3, 1)).squeeze(-1).to(o2)
        raybundle.origins, raybundle.directions = o2, d2

    def apply_to_camera(self, camera) -> Tensor:
        """the corrected sensor-to-world matrix of a Cameras / Lidars object with ``metadata["cam_idx"]``"""
        sensor_to_world = camera.camera_to_worlds if hasattr(camera, "camera_to_worlds") else camera.lidar_to_worlds
        if self.config.mode == "off" or camera.metadata is None or "cam_idx" not in camera.metadata:
            return sensor_to_world
        adj = self(torch.tensor([camera.metadata["cam_idx"]], dtype=torch.long, device=camera.device))
        return torch.cat([torch.bmm(adj[..., :3, :3], sensor_to_world[..., :3, :3]),
                          sensor_to_world[..., :3, 3:] + adj[..., :3, 3:]], dim=-1)

    def get_correction_matrices(self) -> Tensor:
        device = self.pose_adjustment.device if self.config.mode != "off" else self.device
        return self(torch.arange(0, self.num_cameras, device=device).long())

    def get_loss_dict(self, loss_dict: dict) -> None:
        if self.config.mode == "off":
            return
        pa = self._get_pose_adjustment()
        rot = pa[:, 3:].norm(dim=-1).mean() * self.config.rot_l2_penalty
        if self.scaled:
            loss_dict["camera_opt_regularizer"] = (pa[:, :3].abs() * self._trans_penalty).mean() + rot
        else:
            loss_dict["camera_opt_regularizer"] = pa[:, :3].norm(dim=-1).mean() * self.config.trans_l2_penalty + rot

    def get_metrics_dict(self, metrics_dict: dict) -> None:
        """the reference's four keys as 0-dim tensors on the parameter's device (no host read)"""
        if self.config.mode == "off":
            return
        trans = self.pose_adjustment[:, :3].detach().norm(dim=-1)
        rot = self.pose_adjustment[:, 3:].detach().norm(dim=-1)
        metrics_dict["camera_opt_translation_max"] = trans.max()
        metrics_dict["camera_opt_translation_mean"] = trans.mean()
        metrics_dict["camera_opt_rotation_mean"] = rot.mean() * (180.0 / math.pi)
        metrics_dict["camera_opt_rotation_max"] = rot.max() * (180.0 / math.pi)

    def get_param_groups(self, param_groups: dict) -> None:
        params = list(self.parameters())
        if self.config.mode != "off":
            assert len(params) > 0
            param_groups["camera_opt"] = params
        else:
            assert len(params) == 0
