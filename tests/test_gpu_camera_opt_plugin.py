"""The plugin with the fused camera optimizer (``use_fused_camera_optimizer``, what ``fused_camera_opt`` does at build time)
against the plugin without it, both on the GPU, on one training batch with ``camera_optimizer.mode = "SO3xR3"``: the gradient
of every loss term on ``pose_adjustment`` -- through csrc/pose_opt.hip's integer sums on one side, through torch's gather,
exp-map ops and index backward on the other -- held to the tolerance tests/test_gpu_reference_plugin.py holds that parameter
to against the reference (``check_gradients_against_floor``: the term's own fp32 noise floor); and one fused training step's
metrics."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plugin_harness as t  # noqa: E402
import ref_import  # noqa: E402
from conftest import rel_l2  # noqa: E402
from plugin_harness import N, check_gradients_against_floor, per_loss_gradient_errors, ref  # noqa: E402,F401

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_import.reference_available(), reason="no reference (oracle/_ref ships with the lease)")]


def _step(m, b):
    m.zero_grad(set_to_none=True)
    rb = t.bundle(b, "cuda")
    out = m.get_outputs(rb, patch_size=(b["patch"], b["patch"]), calc_lidar_losses=True)
    labels = t.labels(b, "cuda")
    metrics = m.get_metrics_dict(out, labels)
    return rb, out, metrics, m.get_loss_dict(out, labels, metrics)


def test_pose_gradients_per_loss_term_match_the_plugin_without_the_flag(ref):  # noqa: F811
    from neurad_studio_amd.cameras.camera_optimizers import METRIC_KEYS, CameraOptimizer

    on, _ = t.build_pair(ref, False, pose_opt=True)
    off, _ = t.build_pair(ref, False, pose_opt=True)
    pose = on.camera_optimizer.pose_adjustment
    on.use_fused_camera_optimizer()
    assert type(on.camera_optimizer) is CameraOptimizer and on.camera_optimizer.pose_adjustment is pose
    assert type(off.camera_optimizer) is not CameraOptimizer and list(on.state_dict()) == list(off.state_dict())
    b = t.batch(False)
    t.deterministic(on, True), t.deterministic(off, True)
    assert on.fused_training_possible()
    a_rb, a_out, a_met, a_loss = _step(on, b)
    b_rb, b_out, b_met, b_loss = _step(off, b)
    assert a_rb.origins.requires_grad and a_rb.origins.dtype == torch.float32 and a_rb.origins.shape == b_rb.origins.shape
    # two fp32 evaluations, each within 16 * 2^-24 ||d|| per element of float64 (include/neurad_hip.h): 32 * 2^-24 * sqrt(3)
    ray_tol = 32 * 2.0 ** -24 * 3 ** 0.5
    assert rel_l2(N(a_rb.origins), N(b_rb.origins)) < ray_tol and rel_l2(N(a_rb.directions), N(b_rb.directions)) < ray_tol
    assert list(a_loss) == list(b_loss) and "camera_opt_regularizer" in a_loss
    for k in b_loss:
        x, y = float(a_loss[k]), float(b_loss[k])
        assert abs(x - y) <= 2e-4 * abs(y) + 1e-7, (k, x, y)
    errs = per_loss_gradient_errors(on, a_loss, off, b_loss, detail=True)
    pose_errs = {term: {"pose": kinds["pose"]} for term, kinds in errs.items() if "pose" in kinds}
    assert {"rgb_loss", "interlevel_loss", "depth_loss", "camera_opt_regularizer"} <= set(pose_errs), sorted(pose_errs)
    report = check_gradients_against_floor(pose_errs, t.floors("static_pose"))
    print("pose gradient per loss term (rel-L2, bound):", {k: (v["rel_l2"], v["bound"]) for k, v in report.items()})
    # one fused training step's metrics: the four pose keys as device tensors, no host read behind them
    assert list(a_met) == list(b_met)
    for k in METRIC_KEYS:
        assert isinstance(a_met[k], torch.Tensor) and a_met[k].is_cuda and a_met[k].shape == (), k
        assert abs(float(a_met[k]) - float(b_met[k])) <= 1e-5 * abs(float(b_met[k])), k
