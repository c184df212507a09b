"""The plugin's camera image evaluation (``fused_image_eval``) on the CPU: the glue of ``get_image_metrics_and_images`` and of
the training ``get_metrics_dict`` -- the reference's own method bodies with ``self.psnr`` / ``self.ssim`` answered by
model_components/image_metrics.py for the duration of the call, one transfer for the two scalars, the reference's keys,
images and LPIPS untouched, the lidar branch beside it with and without ``fused_lidar_eval``.

On CPU tensors the image metrics run through the module's float64 fallback in place of csrc/image_eval.hip (the kernels are
tested on the GPU: tests/test_gpu_image_eval.py); the lidar branch's chamfer op is answered by tests/lidar_eval_standins.py.
The reference's OWN ``psnr`` / ``ssim`` / ``lpips`` are mocks in this harness, because torchmetrics is stubbed
(oracle/ref_import.py): the two values are therefore compared against the float64 restatement (tests/image_eval_refs.py) on
the same tensors, not against the reference model's numbers; ``images_dict`` IS compared against the reference model's own.
The image is a synthetic stand-in of the shapes an eval render produces (``rgb`` [H,W,3], ``depth`` [H,1]); H equals the scan's
point count so that one ``outputs`` dict can feed the image and the lidar branch at once, as the reference's method allows."""
import os
import sys
from copy import deepcopy

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import image_eval_refs as R  # noqa: E402
import lidar_eval_refs as LR  # noqa: E402
import plugin_harness as t  # noqa: E402
import ref_import  # noqa: E402
import synth  # noqa: E402
from lidar_eval_standins import DeviceStandIns  # noqa: E402
from plugin_harness import N, T, ref  # noqa: E402,F401

pytestmark = pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")
H, W = 40, 23


def _pair(ref_neurad, fused_lidar_eval):
    from nerfstudio.data.scene_box import SceneBox

    def kw():
        return dict(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                    metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}, "trajectories": []})

    mcfg = t.shrink(deepcopy(t.methods()["neurad-hip"].pipeline.model))
    mcfg.fused_decoder, mcfg.fused_lidar_eval, mcfg.fused_image_eval = False, fused_lidar_eval, True
    torch.manual_seed(0)
    hip = mcfg.setup(**kw()).eval()
    ref_cfg = t.shrink(ref_neurad.NeuRADModelConfig(implementation="torch"))
    for c in (ref_cfg.field, ref_cfg.sampling.proposal_field_1, ref_cfg.sampling.proposal_field_2):
        c.grid.actor.use_4d_hashgrid = False
    refm = ref_cfg.setup(**kw()).eval()
    return hip, refm


def _render():
    image, rgb = R.images("smooth", H, W)
    outputs = {"rgb": T(rgb), "depth": T(synth.uniform((H, 1), 2.0, 60.0, 61)), "accumulation": T(synth.uniform((H, 1), 0, 1, 62))}
    return outputs, {"image": T(image)}, image, rgb


def _scan_outputs(outputs, batch):
    g = LR.scan(H, seed=640)
    outputs.update(intensity=T(g["intensity"]), ray_drop_logits=T(g["ray_drop_logits"]), points=T(g["pred_points"]))
    outputs["depth"] = T(g["depth"])
    batch.update(lidar=T(g["points"]), distance=T(g["distance"]), did_return=torch.from_numpy(g["did_return"])[:, None],
                 is_lidar=torch.ones(H, 1, dtype=torch.bool))
    return g


@pytest.fixture
def gray_depth(ref, monkeypatch):  # noqa: F811
    """matplotlib's colour tables are stubbed in this harness: depth images as grey levels, for both models"""
    from nerfstudio.utils import colormaps

    monkeypatch.setattr(colormaps, "apply_depth_colormap", lambda depth, *a, **k: depth.expand(*depth.shape[:-1], 3) / 100.0)


def _count_transfers(hip, monkeypatch):
    transfers = []
    to_host = type(hip)._scalars_to_host
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: (transfers.append(tuple(v.shape)), to_host(v))[1]))
    return transfers


def _check_image_metrics(metrics, image, rgb):
    tol = R.conv_form_float64_error(image, rgb)  # (the fallback: torchmetrics' one-conv2d form in float64)
    assert all(type(metrics[k]) is float for k in ("psnr", "ssim", "lpips"))
    assert abs(metrics["ssim"] - R.ssim_valid(image, rgb).mean()) <= tol
    assert abs(metrics["psnr"] - R.psnr(image, rgb)) <= 1e-12


def test_image_branch_takes_psnr_and_ssim_from_one_transfer(ref, gray_depth, monkeypatch):  # noqa: F811
    hip, refm = _pair(ref, fused_lidar_eval=False)
    outputs, batch, image, rgb = _render()
    transfers = _count_transfers(hip, monkeypatch)
    before = (hip.psnr, hip.ssim, dict(hip._modules), set(hip.__dict__))
    metrics, images = hip.get_image_metrics_and_images(outputs, dict(batch))
    want_metrics, want_images = refm.get_image_metrics_and_images(outputs, dict(batch))
    assert list(metrics) == list(want_metrics) == ["psnr", "ssim", "lpips"]
    _check_image_metrics(metrics, image, rgb)
    assert transfers == [(2,)]
    assert list(images) == list(want_images) == ["img", "depth"]
    for k in images:
        assert torch.equal(images[k], want_images[k]), k
    assert tuple(images["img"].shape) == (H, 2 * W, 3)
    # the model is what it was: the metric objects, the module tree, no attribute left behind
    assert (hip.psnr, hip.ssim, dict(hip._modules), set(hip.__dict__)) == before
    # a failure inside the call restores them as well
    with pytest.raises(KeyError):
        hip.get_image_metrics_and_images({"rgb": outputs["rgb"]}, dict(batch))
    assert (hip.psnr, hip.ssim, set(hip.__dict__)) == (before[0], before[1], before[3])
    with pytest.raises(ValueError):  # below the window: the reference's reflect pad fails there too
        hip.get_image_metrics_and_images({**outputs, "rgb": outputs["rgb"][:, :10]}, {"image": batch["image"][:, :10]})


@pytest.mark.parametrize("fused_lidar_eval", [False, True])
def test_image_and_lidar_in_one_batch(ref, gray_depth, monkeypatch, fused_lidar_eval):  # noqa: F811
    hip, refm = _pair(ref, fused_lidar_eval)
    dev = DeviceStandIns().install(monkeypatch)
    outputs, batch, image, rgb = _render()
    g = _scan_outputs(outputs, batch)
    transfers = _count_transfers(hip, monkeypatch)
    metrics, images = hip.get_image_metrics_and_images(outputs, dict(batch))
    want_metrics, want_images = refm.get_image_metrics_and_images(outputs, dict(batch))
    assert list(metrics) == list(want_metrics) == ["psnr", "ssim", "lpips"] + list(LR.METRIC_KEYS)
    _check_image_metrics(metrics, image, rgb)
    assert transfers == ([(2,), (5,)] if fused_lidar_eval else [(2,)])
    assert [c[0] for c in dev.calls] == (["chamfer_distance"] if fused_lidar_eval else [])
    restated = LR.lidar_metrics(g["depth"], g["intensity"], g["ray_drop_logits"], g["pred_points"], g["points"], g["distance"],
                                g["did_return"], hip.config.loss.ray_drop_loss_mult, hip.config.loss.non_return_lidar_distance)
    for k in LR.METRIC_KEYS:
        assert abs(float(metrics[k]) - float(want_metrics[k])) <= 1e-4 * abs(float(want_metrics[k])), (k, metrics[k], want_metrics[k])
        assert abs(float(metrics[k]) - restated[k]) <= 1e-4 * abs(restated[k]), (k, metrics[k], restated[k])
    for k in images:
        assert torch.equal(images[k], want_images[k]), k


def test_training_psnr_is_a_tensor_without_metric_state(ref, monkeypatch):  # noqa: F811
    hip, _ = _pair(ref, fused_lidar_eval=False)
    outputs, batch, image, rgb = _render()
    called = []
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: called.append("transfer")))
    old = hip.psnr
    hip.train()
    metrics = hip.get_metrics_dict({"rgb": outputs["rgb"].requires_grad_()}, dict(batch))
    assert isinstance(metrics["psnr"], torch.Tensor) and metrics["psnr"].shape == () and not metrics["psnr"].requires_grad
    assert metrics["psnr"].device == outputs["rgb"].device and metrics["psnr"].dtype == torch.float32
    want = R.psnr(image, rgb)
    assert abs(float(metrics["psnr"]) - want) <= R.psnr_bound(want)
    assert called == [] and hip.psnr is old


def test_flag_off_leaves_the_reference_objects_in_charge(ref, gray_depth, monkeypatch):  # noqa: F811
    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModel, NeuRADHipModelConfig
    from neurad_studio_amd.model_components import image_metrics as IM

    assert NeuRADHipModelConfig().fused_image_eval is False
    hip, _ = _pair(ref, fused_lidar_eval=False)
    hip.config.fused_image_eval = False
    outputs, batch, _, _ = _render()
    called = []
    monkeypatch.setattr(NeuRADHipModel, "_scalars_to_host", staticmethod(lambda v: called.append("fused")))
    for name in ("image_eval_metrics", "image_metrics_torch", "image_psnr_torch"):
        monkeypatch.setattr(IM, name, lambda *a, **k: called.append("image_metrics"))
    psnr_calls, ssim_calls = [], []
    hip.__dict__["psnr"] = lambda a, b: psnr_calls.append((a.shape, b.shape)) or torch.tensor(31.0)
    hip.__dict__["ssim"] = lambda a, b: ssim_calls.append((a.shape, b.shape)) or torch.tensor(0.5)
    metrics, _ = hip.get_image_metrics_and_images(outputs, dict(batch))
    assert (metrics["psnr"], metrics["ssim"]) == (31.0, 0.5)
    assert psnr_calls == ssim_calls == [((1, 3, H, W), (1, 3, H, W))]  # the reference's own calls, on its [1,C,H,W] views
    hip.train()
    assert float(hip.get_metrics_dict({"rgb": outputs["rgb"]}, dict(batch))["psnr"]) == 31.0
    assert called == []
