"""``neurad-hip``: NeuRAD with its volumetric hot path on libneurad_hip.so, as a nerfstudio method plugin.

    export NERFSTUDIO_METHOD_CONFIGS="neurad-hip=neurad_studio_amd.integration.neurad_hip:neurad_hip"
    ns-train neurad-hip pandaset-data ...

(or list ``neurad_hip`` under the ``nerfstudio.method_configs`` entry-point group -- plugins/registry.py:34-79).

Nothing of neurad-studio is edited or re-typed: ``NeuRADHipModel`` IS the reference's NeuRADModel
(nerfstudio/models/neurad.py:164) -- same config, decoders, losses, metrics, checkpoints -- with
  * ``field`` / ``proposal_fields`` built from this package's NeuRADField / NeuRADProposalField through the configs'
    ``_target`` (configs/base_config.py:47-54); same state_dict names, so neurad checkpoints load;
  * ``sampler``, the renderers, ``lidar_decoder`` and the two sampler losses replaced by their HIP-backed namesakes
    after ``populate_modules``;
  * ``get_nff_outputs`` running the two fused kernels for eval chunks (FusedEvalMixin), the fused training nodes for
    training steps (FusedTrainMixin: sampler rounds, field + head + compositing + appearance as a handful of autograd
    nodes, same output keys; scenes with dynamic actors run on the same nodes with per-sample row overrides) and the
    reference's OWN ``get_nff_outputs`` (models/neurad.py:368-421) otherwise (``fused_training=False``, options the fused
    nodes do not cover).
Per-actor 3-D grids are used (``use_4d_hashgrid=False``): the 4-D grid exists only inside tiny-cuda-nn.
"""
from __future__ import annotations

import contextlib
import dataclasses
from copy import deepcopy
from dataclasses import dataclass
from typing import Literal, Type

import torch

import nerfstudio.models.neurad as _ref_neurad
from nerfstudio.engine.optimizers import AdamOptimizerConfig, AdamWOptimizerConfig
from nerfstudio.field_components.neurad_encoding import ActorSettings, NeuRADHashEncodingConfig
from nerfstudio.fields.neurad_field import NeuRADFieldConfig, NeuRADProposalFieldConfig
from nerfstudio.models.neurad import NeuRADModel, NeuRADModelConfig, SamplingSettings
from nerfstudio.plugins.types import MethodSpecification

from ..field_components.mlp import MLP as HipMLP
from ..fields.neurad_field import NeuRADField as HipNeuRADField
from ..fields.neurad_field import NeuRADProposalField as HipNeuRADProposalField
from ..model_components import losses as hip_losses
from ..model_components import ray_samplers as hip_samplers
from ..model_components import renderers as hip_renderers
from ..model_components.image_metrics import PSNR, ImageEvalPair, ImageEvalTriple, lpips_eval_metric
from ..model_components.lidar_metrics import lidar_eval_metrics, masked_return_metrics, scalars_to_host
from ..models.neurad import FusedEvalMixin, FusedTrainMixin
from ..optim import HashGridAdam
from ..shims import nerfacc as hip_nerfacc


@dataclass
class HashGridAdamConfig(AdamOptimizerConfig):
    """``hashgrids`` group of the method (configs/method_configs.py:423-426: Adam, lr 1e-2, eps 1e-15) on csrc/adam.hip.  The
    reference builds every optimizer as ``config._target(params, **fields)`` (engine/optimizers.py:39-62) and steps it through
    ``grad_scaler.step`` (engine/optimizers.py:160-181): HashGridAdam takes the scale and the found-inf flag from the
    GradScaler on the device (optim.py), so neither the 0.6 GB of table gradients get an unscale pass nor do fp16 gradients
    (``table_dtype="float16"``) trip ``GradScaler.unscale_``."""

    _target: Type = HashGridAdam
    capturable: bool = False
    """step counts on the device from the first step (a training step captured in a HIP graph)"""


def _field_config() -> NeuRADFieldConfig:
    """the reference's default main-field config (fields/neurad_field.py:46-52) -> HIP field, 3-D actor grids"""
    return NeuRADFieldConfig(_target=HipNeuRADField, grid=NeuRADHashEncodingConfig(
        require_actor_grad=True, actor=ActorSettings(flip_prob=0.25, use_4d_hashgrid=False)))


def _proposal_config() -> NeuRADProposalFieldConfig:
    cfg = NeuRADProposalFieldConfig()  # the reference's defaults (fields/neurad_field.py:158-179)
    cfg._target = HipNeuRADProposalField
    cfg.grid.actor.use_4d_hashgrid = False
    return cfg


def _sampling() -> SamplingSettings:
    return SamplingSettings(proposal_field_1=_proposal_config(), proposal_field_2=_proposal_config())


@dataclass
class FusedAdamConfig(AdamOptimizerConfig):
    """the small groups' torch.optim.Adam with ``fused=True``: one multi-tensor launch per group, and -- like HashGridAdam --
    an optimizer that takes the GradScaler's scale / found-inf on the device, where the reference's default (foreach) Adam
    makes ``GradScaler.step`` read found-inf back to the host for every optimizer and iteration (torch/amp/grad_scaler.py
    `_maybe_opt_step`: a ``.item()``)"""

    fused: bool = True


@dataclass
class FusedAdamWConfig(AdamWOptimizerConfig):
    fused: bool = True


@dataclass
class NeuRADHipModelConfig(NeuRADModelConfig):
    _target: Type = dataclasses.field(default_factory=lambda: NeuRADHipModel)
    sampling: SamplingSettings = dataclasses.field(default_factory=_sampling)
    field: NeuRADFieldConfig = dataclasses.field(default_factory=_field_config)  # (shadows dataclasses.field below)
    fused_eval: bool = True
    """Eval chunks through the two fused kernels (False: operator-level path everywhere)."""
    fused_decoder: bool = True
    """decode_features' RGB CNN decoder on csrc/decoder.hip (False: the torch modules)."""
    early_stop_eps: float = 0.0
    """> 0: eval rays stop marching once their transmittance is below it (bounded error); 0 = exact."""
    order_rays: bool = False
    """Cache-coherent processing order per eval chunk (pays for lidar scans / random pixels, not for image patches)."""
    fused_training: bool = True
    """Training steps of a static scene on the fused nodes (models/neurad.py FusedTrainMixin); False: the reference's own
    get_nff_outputs over the HIP modules."""
    fused_losses: bool = True
    """Training steps: the lidar terms of get_metrics_dict (models/neurad.py:485-521) on csrc/losses.hip (one launch each way,
    the quantile as a radix select) and every per-step metric without boolean-mask indexing -- the reference's formulation
    costs ~15 `x[mask]` (a nonzero + a device->host read each) and a `float(beta)` per step, which serialise the host with the
    GPU.  Same keys, same values (tests/test_gpu_reference_plugin.py); False: the reference's own get_metrics_dict."""
    fused_lidar_eval: bool = False
    """Evaluation of a lidar scan (``ns-eval``, in-training eval) on the device: get_outputs_for_lidar builds its rays with
    cameras/raygen.py:lidar_rays, the lidar branch of get_image_metrics_and_images (models/neurad.py:589-620) runs as masked
    reductions plus the chamfer kernel (csrc/lidar_eval.hip) and reads its five scalars with one device->host transfer.
    False: the reference's own methods (torch ray generation, ~8 boolean-mask gathers, chunked torch.cdist)."""
    median_depth: bool = False
    """Eval outputs also carry ``median_depth`` [R,1] (csrc/median_depth.hip): the midpoint of the first non-sky sample at
    which the accumulated weight reaches one half -- the reference's DepthRenderer("median") with its CPU numerics, one more
    launch per eval chunk.  Only the fused eval route produces the key (``fused_eval``; training outputs do not have it).
    With ``fused_lidar_eval`` a scan's outputs gain ``median_points`` and its metrics ``median_depth_median_l2``,
    ``median_depth_mean_rel_l2`` and ``median_chamfer_distance`` (SplatAD's names), all eight scalars in the one transfer.
    False: no key, launch or host read changes."""
    normals: bool = False
    """Eval outputs also carry ``normals`` [R,3] (csrc/normals.hip): the weighted sum of the non-sky samples' unit normals of
    the geometry head (the SDF's gradient, towards free space; its negative in density mode), normalised as the
    reference's NormalsRenderer does; one more launch per eval chunk.  Only the fused eval route produces the key.  With
    dynamic actors a sample inside a box contributes that actor's normal, rotated to the world, at the ray's time (the
    bundle's ``times``; the render's candidate lists are shared).  False: no key, no launch."""
    fused_image_eval: bool = False
    """Camera image metrics on the device (csrc/image_eval.hip, model_components/image_metrics.py): the image branch of
    get_image_metrics_and_images (models/neurad.py:568-587) takes ``psnr`` and ``ssim`` from one launch sequence and reads both
    with one device->host transfer (``lpips`` and the images stay the reference's), and the training step's ``psnr``
    (models/neurad.py:465) is ``ops.image_psnr``: a device tensor, no torchmetrics module state.  False: the reference's
    torchmetrics objects (a ``float()`` per metric; SSIM as a grouped conv2d with fp32 E[x^2] - mu^2 variances)."""
    fused_lpips: bool = False
    """LPIPS on the device (csrc/lpips.hip, model_components/lpips.py): ``self.lpips`` adopts the reference object's network
    (``LPIPS.from_reference``: no tensor copied, the state dict stays the reference's) and the ``lpips`` of
    get_image_metrics_and_images (models/neurad.py:587) is AlexNet on the fp16 matrix cores, its value and the flag of
    torchmetrics' value-range check read with one transfer.  Together with ``fused_image_eval`` all three image metrics share
    ONE transfer.  False: the reference's torchmetrics object (fp32 through the vendor library, two host reads)."""
    fused_camera_opt: bool = False
    """Camera pose correction on the device (csrc/pose_opt.hip, cameras/camera_optimizers.py): with
    ``camera_optimizer.mode = "SO3xR3"`` (the `*-scaleopt` methods) ``self.camera_optimizer`` becomes this package's
    CameraOptimizer around the reference module's own Parameter and ``weights`` buffer (same state-dict names, parameter
    group and checkpoints).  ``apply_to_raybundle`` is one autograd node -- one launch forwards; backwards per-camera integer
    sums, bit-identical for any order of the rays -- and ``get_metrics_dict`` returns device tensors (the reference's
    ``rot.mean().cpu()`` / ``rot.max().cpu()`` are two host synchronisations per step).  Deviation under AMP: the corrected
    directions stay fp32, where the reference's ``torch.bmm`` under autocast rounds them through fp16.  False, mode "off",
    mode "SE3" or ``non_trainable_camera_indices``: the reference's module."""
    table_dtype: Literal["float32", "float16"] = "float32"
    """Storage of the main field's hash tables (static grid + actor grids).  "float16" (BASELINE config[4]; what tiny-cuda-nn
    stores): half the gather bytes; gradients arrive in fp16 and HashGridAdam keeps fp32 master copies (optim.py).  State
    dicts load into either (load_state_dict casts), so fp32 neurad checkpoints interchange."""
    proposal_table_dtype: Literal["float32", "float16"] = "float32"
    """... and of the proposal fields' static tables (their actor grids stay fp32: the fused sampler reads those as fp32)."""
    fused_vgg_loss: bool = False
    """The VGG perceptual term (``loss.vgg_mult``, models/neurad.py:260,537-538) as one autograd node on csrc/vgg_loss.hip
    (model_components/perceptual.py): ``self.vgg_loss`` adopts the reference module's tensors, so the state dict and
    ``get_loss_dict`` stay the reference's.  False: the reference's torch module (MIOpen under autocast)."""


class _NchwDecoderAdapter(torch.nn.Module):
    """what the reference's decode_features calls in place of ``self.rgb_decoder`` (models/neurad.py:362-365): it receives
    the NCHW VIEW of the pixel-major feature rows and hands an NCHW view of the pixel-major result back, so neither permute
    moves a byte, and the convolutions run on csrc/decoder.hip (model_components/cnns.py:decode_rgb)."""

    def __init__(self, decoder):
        super().__init__()
        self.__dict__["decoder"] = decoder  # not a registered submodule: the state_dict stays the reference's

    def forward(self, x):
        from neurad_studio_amd.model_components.cnns import decode_rgb

        b, c, h, w = x.shape
        return decode_rgb(self.decoder, x.permute(0, 2, 3, 1).reshape(-1, c).float(), (h, w)).permute(0, 3, 1, 2)


@contextlib.contextmanager
def _patched(module, name, value):
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


@contextlib.contextmanager
def _shadowed(obj, **values):
    """instance attributes for the duration of a call, whatever they shadow: a plain attribute, a class attribute or a
    registered submodule (``obj._modules`` and the state dict stay as they are: the instance dict is looked up first)"""
    d, missing = obj.__dict__, object()
    old = {k: d.get(k, missing) for k in values}
    d.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is missing:
                d.pop(k, None)
            else:
                d[k] = v


class NeuRADHipModel(FusedEvalMixin, FusedTrainMixin, NeuRADModel):
    config: NeuRADHipModelConfig
    reference_output_keys = True  # get_metrics_dict consumes outputs["non_nearby_weights"] (models/neurad.py:508)

    def populate_modules(self):
        super().populate_modules()  # fields come out of config._target -> this package's classes
        cfg = self.config
        assert isinstance(self.field, HipNeuRADField), "config.field._target must be the HIP NeuRADField"
        self.fused_eval, self.early_stop_eps, self.order_rays = cfg.fused_eval, cfg.early_stop_eps, cfg.order_rays
        self.fused_training, self.median_depth, self.normals = cfg.fused_training, cfg.median_depth, cfg.normals
        if cfg.fused_vgg_loss:
            from neurad_studio_amd.model_components.perceptual import VGGPerceptualLoss

            self.vgg_loss = VGGPerceptualLoss.from_reference(self.vgg_loss)
        if cfg.fused_lpips:
            from neurad_studio_amd.model_components.lpips import LPIPS

            self.lpips = LPIPS.from_reference(self.lpips)
        if cfg.fused_camera_opt:
            self.use_fused_camera_optimizer()
        s = cfg.sampling
        self.sampler = hip_samplers.ProposalNetworkSampler(
            num_proposal_samples_per_ray=s.num_proposal_samples, num_nerf_samples_per_ray=s.num_nerf_samples,
            num_proposal_network_iterations=cfg.num_proposal_rounds, single_jitter=s.single_jitter,
            initial_sampler=hip_samplers.PowerSampler(lambda_=s.power_lambda, scaling=s.power_scaling),
            update_sched=lambda x: 0)
        self.lidar_decoder = HipMLP(in_dim=cfg.field.nff_out_dim + cfg.appearance_dim, layer_width=32, out_dim=2,
                                    num_layers=3, out_activation=None)
        self.renderer_feat = hip_renderers.FeatureRenderer()
        self.renderer_accumulation = hip_renderers.AccumulationRenderer()
        self.renderer_depth = (hip_renderers.DepthRenderer(method="expected") if cfg.normalize_depth
                               else hip_renderers.render_depth_simple)
        self.interlevel_loss = hip_losses.zipnerf_interlevel_loss
        for what, name in ((cfg.table_dtype, "table_dtype"), (cfg.proposal_table_dtype, "proposal_table_dtype")):
            if what not in ("float32", "float16"):
                raise ValueError(f"{name} must be 'float32' or 'float16', got {what!r}")
        if cfg.table_dtype == "float16":
            for gr in [self.field.hashgrid.static_grid, *self.field.hashgrid.actor_grids]:
                gr.hash_table.data = gr.hash_table.data.half()
        if cfg.proposal_table_dtype == "float16":
            for pf in self.proposal_fields:
                pf.hashgrid.static_grid.hash_table.data = pf.hashgrid.static_grid.hash_table.data.half()

    def use_fused_camera_optimizer(self) -> None:
        """``config.fused_camera_opt`` for a model that is already built: swaps ``self.camera_optimizer`` for
        cameras/camera_optimizers.py:CameraOptimizer around the same Parameter object (idempotent; the reference's module
        stays where that class does not restate it)"""
        from ..cameras.camera_optimizers import CameraOptimizer

        self.camera_optimizer = CameraOptimizer.from_reference(self.camera_optimizer)

    def _render_weights(self, outputs, ray_samples):
        """models/neurad.py:711-724 without the cpu placeholder and independent of which ``nerfacc`` is importable"""
        with _patched(_ref_neurad, "nerfacc", hip_nerfacc):
            return super()._render_weights(outputs, ray_samples)

    def get_nff_outputs(self, ray_bundle, calc_lidar_losses: bool = False):
        if self.fused_eval_possible():
            return self.fused_nff_outputs(ray_bundle)
        if self.fused_training_possible():
            return self._fused_train_nff_outputs(ray_bundle, calc_lidar_losses)
        return super().get_nff_outputs(ray_bundle, calc_lidar_losses)

    _batch_layout = None

    def set_batch_layout(self, n_camera_rays, n_lidar_rays) -> None:
        """The caller vouches that the NEXT bundle is [n_camera_rays camera rays; n_lidar_rays lidar rays] in this order --
        what ``_merge_img_lidar`` builds (data/datamanagers/image_lidar_datamanager.py:379-423).  ``decode_features`` then
        splits the rendered features with two views instead of two boolean-mask gathers (each a nonzero + a host read).
        Set by integration/pipeline.py:ADHipPipeline, which owns the batch; consumed once."""
        self._batch_layout = None if n_camera_rays is None else (int(n_camera_rays), int(n_lidar_rays))

    def decode_features(self, features, patch_size, is_lidar=None, intensity_for_cam=False):
        """the reference's method (models/neurad.py:337-366) with the RGB CNN decoder on the HIP kernels: fp16 operands, fp32
        accumulation -- what the reference's mixed-precision trainer runs through MIOpen"""
        layout, self._batch_layout = self._batch_layout, None
        if self._all_lidar_bundle:
            # a whole lidar scan (get_outputs_for_lidar): every row goes to the lidar head; models/neurad.py:348-365 would
            # gather by two boolean masks and run the CNN decoder on an empty batch
            intensity, ray_drop_logit = self.lidar_decoder(features).float().split(1, dim=-1)
            return None, intensity.sigmoid(), ray_drop_logit
        if (layout is not None and is_lidar is not None and not intensity_for_cam and features.is_cuda
                and sum(layout) == features.shape[0] and layout[0] > 0 and layout[1] > 0):
            # models/neurad.py:345-366 with the two masks replaced by the layout's views
            n_cam = layout[0]
            intensity, ray_drop_logit = self.lidar_decoder(features[n_cam:]).split(1, dim=-1)
            cam = features[:n_cam]
            if self.config.fused_decoder:
                from neurad_studio_amd.model_components.cnns import decode_rgb

                rgb = decode_rgb(self._modules["rgb_decoder"], cam.float(), tuple(patch_size))
            else:
                rgb = self.rgb_decoder(cam.view(-1, *patch_size, cam.shape[-1]).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
            return rgb, intensity.sigmoid(), ray_drop_logit
        if not (self.config.fused_decoder and features.is_cuda):
            return super().decode_features(features, patch_size, is_lidar, intensity_for_cam)
        decoder = self._modules["rgb_decoder"]
        self._modules["rgb_decoder"] = _NchwDecoderAdapter(decoder)
        try:
            return super().decode_features(features, patch_size, is_lidar, intensity_for_cam)
        finally:
            self._modules["rgb_decoder"] = decoder

    def get_metrics_dict(self, outputs, batch):
        if (self.training and self.config.fused_losses and "lidar" in batch and "image" in batch
                and outputs["depth"].is_cuda and "weights_list" in outputs):
            return self._fused_metrics_dict(outputs, batch)
        # the reference calls the module-level distortion_loss (models/neurad.py:524): the HIP one for this call only
        with _patched(_ref_neurad, "distortion_loss", hip_losses.distortion_loss):
            if self.config.fused_image_eval and "image" in batch:
                with _shadowed(self, psnr=PSNR(1.0)):  # (models/neurad.py:265: data_range=1.0)
                    return super().get_metrics_dict(outputs, batch)
            return super().get_metrics_dict(outputs, batch)

    def _fused_metrics_dict(self, outputs, batch):
        """get_metrics_dict (models/neurad.py:461-529) of a training step without a device->host read: same keys, same
        values.  The number of lidar rays comes with the batch (``batch["lidar"]`` has one row per lidar ray), so their
        positions are a compaction with a known size (ops.mask_compact) instead of a nonzero; the depth / intensity / ray-drop
        terms of the final samples and the depth terms of both proposal rounds are one launch each way (csrc/losses.hip); the
        four logging metrics are masked reductions."""
        from ..model_components.lidar_losses import LidarLossSettings, lidar_metrics, lidar_rows

        loss = self.config.loss
        if self.config.fused_image_eval:  # a 0-dim device tensor from csrc/image_eval.hip: no metric object, no host read
            m = {"psnr": PSNR(1.0)(outputs["rgb"].detach(), batch["image"])}
        else:
            m = {"psnr": self.psnr(outputs["rgb"].detach(), batch["image"])}
        is_lidar = batch["is_lidar"][:, 0]
        n_lidar = batch["lidar"].shape[0]
        rows = lidar_rows(is_lidar, n_lidar)
        did_return = batch["did_return"].index_select(0, rows[0])[:, 0]
        target_i, distance = batch["lidar"][..., 3:4], batch["distance"]
        with torch.no_grad():  # the four eval metrics the reference logs every step (models/neurad.py:477-483)
            pred = outputs["depth"].detach().index_select(0, rows[0])
            m.update(masked_return_metrics(pred, distance, outputs["intensity"].detach(), target_i,
                                            outputs["ray_drop_logits"].detach(), did_return))
        cfg = LidarLossSettings(depth_mult=loss.depth_mult, intensity_mult=loss.intensity_mult, carving_mult=loss.carving_mult,
                                quantile_threshold=loss.quantile_threshold,
                                non_return_lidar_distance=loss.non_return_lidar_distance,
                                non_return_loss_mult=loss.non_return_loss_mult, ray_drop_loss_mult=loss.ray_drop_loss_mult,
                                prop_lidar_loss_mult=loss.prop_lidar_loss_mult)
        m.update(lidar_metrics(outputs, is_lidar, did_return, distance, target_i, cfg,
                               num_proposal_rounds=self.config.num_proposal_rounds, rows=rows))
        m["distortion"] = hip_losses.distortion_loss(outputs["weights_list"], outputs["ray_samples_list"])
        if self.config.field.use_sdf:
            m["sdf_to_density"] = self.field.sdf_to_density.beta.detach()  # (the reference: float(beta), a host read per step)
        self.camera_optimizer.get_metrics_dict(m)
        return m

    # ---- evaluation of a lidar scan (fused_lidar_eval) ---------------------------------------------------------------------
    _all_lidar_bundle = False

    @torch.no_grad()
    def get_outputs_for_lidar(self, lidar, batch):
        """models/ad_model.py:85-114 with the rays from the device generator (cameras/raygen.py:lidar_rays, in the reference's
        RayBundle class) and the whole scan through the lidar head without a mask gather; the render itself is the reference's
        chunk loop (get_outputs_for_camera_ray_bundle) over the fused eval kernels.  Same keys as the reference except "rgb",
        which the reference fills with an empty tensor for a scan."""
        if not self.config.fused_lidar_eval:
            return super().get_outputs_for_lidar(lidar, batch)
        from nerfstudio.cameras.rays import RayBundle
        from nerfstudio.utils.poses import inverse as pose_inverse

        from ..cameras.raygen import lidar_rays

        assert isinstance(batch["lidar_idx"], int), "All lidar points are assumed to be from the same scan."
        dev = self.device
        points, lidar = batch["lidar"].to(dev), lidar.to(dev)
        n = points.shape[0]
        ray_bundle = lidar_rays(lidar, torch.zeros((n, 1), dtype=torch.long, device=dev), points, bundle_cls=RayBundle)
        ray_bundle.camera_indices = torch.full((n, 1), batch["lidar_idx"], dtype=torch.long, device=dev)
        batch["is_lidar"] = ray_bundle.metadata["is_lidar"]
        batch["distance"] = ray_bundle.metadata["directions_norm"]
        batch["did_return"] = ray_bundle.metadata["did_return"]
        self._all_lidar_bundle = True
        try:
            outputs = self.get_outputs_for_camera_ray_bundle(ray_bundle)
        finally:
            self._all_lidar_bundle = False
        # points in the lidar's frame (models/ad_model.py:108-113)
        w2l = pose_inverse(lidar.lidar_to_worlds[0])
        for points, depth in (("points", "depth"), ("median_points", "median_depth")):
            if depth in outputs:  # ("median_depth": with config.median_depth, from the fused eval chunks)
                world = ray_bundle.origins + ray_bundle.directions * outputs[depth]
                outputs[points] = (w2l @ torch.cat([world, torch.ones_like(world[..., :1])], dim=-1).unsqueeze(-1)).squeeze(-1)
        return outputs, batch

    def get_image_metrics_and_images(self, outputs, batch):
        """With ``fused_image_eval`` the image branch (models/neurad.py:568-587) runs the reference's own code with
        ``self.psnr`` / ``self.ssim`` answered, for this call, by model_components/image_metrics.py:ImageEvalPair: the first of
        the two launches the image kernels and reads both scalars with one transfer (``_scalars_to_host``), the second is
        served from it.  Same keys, every value a Python float; ``images_dict`` and ``lpips`` are the reference's.
        With ``fused_lpips`` as well, ``self.lpips`` is answered by the same object (ImageEvalTriple) and the three share the one
        transfer; with ``fused_lpips`` alone only ``lpips`` is replaced (its value and range flag in one transfer)."""
        cfg = self.config
        if "image" not in batch or not (cfg.fused_image_eval or cfg.fused_lpips):
            return self._image_and_lidar_metrics(outputs, batch)
        to_host = lambda values: self._scalars_to_host(values)  # noqa: E731
        if not cfg.fused_lpips:
            pair = ImageEvalPair(to_host=to_host)
            shadows = dict(psnr=pair.psnr, ssim=pair.ssim)
        elif not cfg.fused_image_eval:
            module = self.lpips
            shadows = dict(lpips=lambda preds, target: lpips_eval_metric(preds, target, module, to_host=to_host))
        else:
            triple = ImageEvalTriple(self.lpips, to_host=to_host)
            shadows = dict(psnr=triple.psnr, ssim=triple.ssim, lpips=triple.lpips)
        with _shadowed(self, **shadows):
            return self._image_and_lidar_metrics(outputs, batch)

    def _image_and_lidar_metrics(self, outputs, batch):
        """The image branch is the reference's; with ``fused_lidar_eval`` the lidar branch (models/neurad.py:589-620) is
        ``_fused_lidar_eval_metrics``: the same five keys (plus the three of the median depth with ``median_depth``), every
        value a Python float -- the reference returns a 0-dim tensor
        for ``chamfer_distance`` in its fallback case (nothing predicted to return, or nothing returned), this path a float."""
        if not (self.config.fused_lidar_eval and "lidar" in batch and outputs["depth"].shape[0] == batch["lidar"].shape[0]):
            return super().get_image_metrics_and_images(outputs, batch)
        metrics, images = super().get_image_metrics_and_images(outputs, {k: v for k, v in batch.items() if k != "lidar"})
        metrics.update(self._fused_lidar_eval_metrics(outputs, batch))
        return metrics, images

    def _fused_lidar_eval_metrics(self, outputs, batch):
        """every ray of ``outputs`` is a ray of the scan ``batch["lidar"]`` (what get_outputs_for_lidar renders):
        model_components/lidar_metrics.py:lidar_eval_metrics with this model's loss settings; where the outputs carry
        ``median_depth`` and ``median_points`` (``config.median_depth``) the three LIDAR_EVAL_MEDIAN_KEYS come with it"""
        dev, loss = self.device, self.config.loss
        points = batch["lidar"].to(dev)
        for key in ("is_lidar", "did_return"):  # (models/neurad.py:591-594)
            if key not in batch:
                batch[key] = torch.ones(points.shape[0], 1, dtype=torch.bool, device=dev)
        return lidar_eval_metrics(outputs, points, batch["distance"].to(dev), batch["did_return"][:, 0].to(dev),
                                  loss.ray_drop_loss_mult, loss.non_return_lidar_distance, to_host=self._scalars_to_host)

    @staticmethod
    def _scalars_to_host(values):
        """THE device->host transfer of the fused eval metrics: one per lidar scan (five scalars; eight with
        ``median_depth``), one per camera image (two;
        four with ``fused_lpips``: the three metrics and LPIPS' range flag);
        tests count the calls"""
        return scalars_to_host(values)


def _trainer_config():
    # imported here, not at module level: nerfstudio.configs.method_configs runs the plugin discovery at its end
    # (plugins/registry.py:56-73), which imports THIS module -- at module level that is a cycle whenever this module is
    # imported before the method table
    from nerfstudio.configs.method_configs import method_configs

    cfg = deepcopy(method_configs["neurad"])  # schedules, data manager, the small groups' optimizers: the reference's own
    cfg.method_name = "neurad-hip"
    ref_model = cfg.pipeline.model
    cfg.pipeline.model = NeuRADHipModelConfig(eval_num_rays_per_chunk=ref_model.eval_num_rays_per_chunk,
                                              camera_optimizer=ref_model.camera_optimizer)
    # the pipeline: batches drawn on the device, gradients exchanged by GradientSynchronizer instead of DDP
    # (integration/pipeline.py); every field of the reference's pipeline / data manager config is carried over
    from .pipeline import ADHipDataManagerConfig, ADHipPipelineConfig

    ref_pipe, ref_dm = cfg.pipeline, cfg.pipeline.datamanager
    dm = ADHipDataManagerConfig(**{f.name: getattr(ref_dm, f.name) for f in dataclasses.fields(ref_dm)
                                   if f.name not in ("_target", "num_processes")})
    cfg.pipeline = ADHipPipelineConfig(**{f.name: getattr(ref_pipe, f.name) for f in dataclasses.fields(ref_pipe)
                                          if f.name not in ("_target", "datamanager")}, datamanager=dm)
    # the tables' optimizer on the HIP kernel, with the group's own hyper-parameters (configs/method_configs.py:423-426)
    ref_opt = cfg.optimizers["hashgrids"]["optimizer"]
    cfg.optimizers["hashgrids"]["optimizer"] = HashGridAdamConfig(lr=ref_opt.lr, eps=ref_opt.eps, max_norm=ref_opt.max_norm,
                                                                  weight_decay=ref_opt.weight_decay)
    # the small groups (MLPs, CNN decoder, trajectories, camera poses): the reference's optimizers and hyper-parameters, fused
    for name, group in cfg.optimizers.items():
        opt = group["optimizer"]
        if name != "hashgrids" and type(opt) in (AdamOptimizerConfig, AdamWOptimizerConfig):
            fused = FusedAdamWConfig if isinstance(opt, AdamWOptimizerConfig) else FusedAdamConfig
            group["optimizer"] = fused(lr=opt.lr, eps=opt.eps, max_norm=opt.max_norm, weight_decay=opt.weight_decay)
    # the trainer: the reference's iteration without its two grad_scaler.get_scale() host reads (integration/trainer.py)
    from .trainer import HipTrainerConfig

    return HipTrainerConfig(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg) if f.name != "_target"})


_SPEC = None


def __getattr__(name):
    """``neurad_hip`` (the MethodSpecification the registry looks up) is built on first access"""
    global _SPEC
    if name != "neurad_hip":
        raise AttributeError(name)
    if _SPEC is None:
        spec = MethodSpecification(config=_trainer_config(),
                                   description="NeuRAD with the volumetric hot path on MI355X HIP kernels (libneurad_hip.so)")
        if _SPEC is None:  # (building it may have run the discovery, which built it already)
            _SPEC = spec
    return _SPEC
