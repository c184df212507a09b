"""The plugin with ``fused_camera_opt`` on against the plugin with it off, on the CPU, on one training batch with
``camera_optimizer.mode = "SO3xR3"``: same loss-dict keys and values, same gradient on ``pose_adjustment``, same state dict, same
metrics keys.

The device is stood in for by tests/train_step_standins.py (the fused nodes' forward entry points answered by the oracle, the
lidar head's MLP by torch); the distortion and interlevel losses are the reference's own functions.  The stand-ins have no backward (the fused nodes' backward passes are kernels), so on the CPU the
rendering losses cannot be taken back to the rays: the gradient compared here is the one this path CAN form, the
regulariser's.  The gradient through the rays is tests/test_gpu_camera_opt_plugin.py's, on the GPU.  On CPU tensors
``apply_to_raybundle`` runs the module's torch restatement in place of csrc/pose_opt.hip (tests/test_gpu_camera_opt.py)."""
import os
import sys
from copy import deepcopy

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plugin_harness as t  # noqa: E402
import ref_import  # noqa: E402
import synth  # noqa: E402
from plugin_harness import N, T, ref  # noqa: E402,F401
from train_step_standins import TrainStepStandIns  # noqa: E402

pytestmark = pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")


@pytest.fixture
def cpu_device(ref, monkeypatch):  # noqa: F811
    import nerfstudio.model_components.losses as ref_losses

    from neurad_studio_amd.model_components import losses as hip_losses

    TrainStepStandIns().install(monkeypatch)
    monkeypatch.setattr(hip_losses, "distortion_loss", ref_losses.distortion_loss)
    return ref_losses


def _model(flag, scaled=False):
    from nerfstudio.data.scene_box import SceneBox

    mcfg = t.shrink(deepcopy(t.methods()["neurad-hip"].pipeline.model))
    mcfg.fused_decoder, mcfg.fused_camera_opt = False, flag
    if scaled:
        from nerfstudio.cameras.camera_optimizers import ScaledCameraOptimizerConfig

        mcfg.camera_optimizer = ScaledCameraOptimizerConfig(mode="SO3xR3", weights=(1.0, 1.0, 0.01, 0.01, 0.01, 1.0))
    else:
        mcfg.camera_optimizer = deepcopy(mcfg.camera_optimizer)
        mcfg.camera_optimizer.mode = "SO3xR3"
    torch.manual_seed(0)
    m = mcfg.setup(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                   metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}, "trajectories": []})
    t.fill(m)
    pa = m.camera_optimizer.pose_adjustment
    pa.data = T(synth.normal(tuple(pa.shape), seed=55) * np.float32(0.02 * (50.0 if scaled else 1.0)))
    return t.deterministic(m, True)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_flag_on_equals_flag_off_on_a_training_batch(cpu_device, scaled):
    from neurad_studio_amd.cameras.camera_optimizers import METRIC_KEYS, CameraOptimizer
    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModelConfig

    assert NeuRADHipModelConfig().fused_camera_opt is False
    on, off = _model(True, scaled), _model(False, scaled)
    assert type(on.camera_optimizer) is CameraOptimizer and type(off.camera_optimizer) is not CameraOptimizer
    assert list(on.state_dict()) == list(off.state_dict())
    assert ("camera_optimizer.weights" in on.state_dict()) == scaled and "camera_optimizer.pose_adjustment" in on.state_dict()
    for k, v in off.state_dict().items():
        assert torch.equal(on.state_dict()[k], v), k
    assert [p is on.camera_optimizer.pose_adjustment for p in on.get_param_groups()["camera_opt"]] == [True]
    b = t.batch(False)
    res = {}
    for name, m in (("on", on), ("off", off)):
        m.interlevel_loss = cpu_device.zipnerf_interlevel_loss
        m.zero_grad(set_to_none=True)
        rb = t.bundle(b, "cpu")
        outputs = m.get_outputs(rb, patch_size=(b["patch"], b["patch"]), calc_lidar_losses=True)
        assert rb.origins.requires_grad and rb.directions.requires_grad and rb.origins.shape == (len(b["o"]), 3)
        lab = t.labels(b, "cpu")
        metrics = m.get_metrics_dict(outputs, lab)
        loss = m.get_loss_dict(outputs, lab, metrics)
        pose = m.camera_optimizer.pose_adjustment
        grads = torch.autograd.grad(loss["camera_opt_regularizer"], [pose])[0]
        res[name] = (rb, metrics, loss, grads)
    (rb_a, met_a, loss_a, g_a), (rb_b, met_b, loss_b, g_b) = res["on"], res["off"]
    assert t.rel_l2(N(rb_a.origins), N(rb_b.origins)) < 1e-6 and t.rel_l2(N(rb_a.directions), N(rb_b.directions)) < 1e-6
    assert list(loss_a) == list(loss_b) and "camera_opt_regularizer" in loss_a
    for k in loss_b:
        x, y = float(loss_a[k]), float(loss_b[k])
        assert abs(x - y) <= 1e-4 * abs(y), (k, x, y)
    assert list(met_a) == list(met_b) and set(METRIC_KEYS) <= set(met_a)
    for k in METRIC_KEYS:
        assert isinstance(met_a[k], torch.Tensor) and met_a[k].shape == ()
        assert abs(float(met_a[k]) - float(met_b[k])) <= 1e-4 * abs(float(met_b[k])), k
    assert g_a.shape == g_b.shape == (2, 6) and t.rel_l2(N(g_a), N(g_b)) < 1e-4
    assert list(on.state_dict()) == list(off.state_dict())


def test_swapping_a_built_model_is_idempotent_and_leaves_the_other_modes_alone(cpu_device):
    from neurad_studio_amd.cameras.camera_optimizers import CameraOptimizer

    m = _model(False)
    before, pose = m.camera_optimizer, m.camera_optimizer.pose_adjustment
    names = list(m.state_dict())
    m.use_fused_camera_optimizer()
    first = m.camera_optimizer
    m.use_fused_camera_optimizer()
    assert type(first) is CameraOptimizer and m.camera_optimizer is first and first.pose_adjustment is pose
    assert list(m.state_dict()) == names and before is not first
    from nerfstudio.data.scene_box import SceneBox

    mcfg = t.shrink(deepcopy(t.methods()["neurad-hip"].pipeline.model))  # the method's own default: mode "off"
    mcfg.fused_camera_opt = True
    off = mcfg.setup(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                     metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}, "trajectories": []})
    assert mcfg.camera_optimizer.mode == "off" and type(off.camera_optimizer) is not CameraOptimizer
