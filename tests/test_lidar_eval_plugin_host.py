"""The plugin's lidar-scan evaluation (``fused_lidar_eval``) on the CPU, with stand-ins for the device: the glue of
``get_outputs_for_lidar`` and ``get_image_metrics_and_images`` -- bundle, batch keys, chunk loop, lidar head without mask
gathers, points in the lidar frame, the five metrics and their one transfer -- against the REFERENCE's own two methods
(models/ad_model.py:85-114, models/neurad.py:589-620) on the reference model with the same weights.  The device entry points
are answered by tests/lidar_eval_standins.py (the oracle, the reference's ray generator, a torch chamfer with direct
differences); the kernels themselves are tested on the GPU (tests/test_gpu_lidar_eval.py)."""
import os
import sys
from copy import deepcopy

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lidar_eval_refs as R  # noqa: E402
import plugin_harness as t  # noqa: E402
import ref_import  # noqa: E402
import synth  # noqa: E402
from conftest import rel_l2  # noqa: E402
from lidar_eval_standins import DeviceStandIns  # noqa: E402
from plugin_harness import N, T, ref  # noqa: E402,F401

pytestmark = pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")
PTS = 96


def _pair(ref_neurad):
    import nerfstudio.model_components.renderers as ref_renderers
    from nerfstudio.data.scene_box import SceneBox

    def kw():
        return dict(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                    metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}, "trajectories": []})

    mcfg = t.shrink(deepcopy(t.methods()["neurad-hip"].pipeline.model))
    mcfg.fused_decoder, mcfg.fused_lidar_eval = False, True
    torch.manual_seed(0)
    hip = mcfg.setup(**kw()).eval()
    ref_cfg = t.shrink(ref_neurad.NeuRADModelConfig(implementation="torch"))
    for c in (ref_cfg.field, ref_cfg.sampling.proposal_field_1, ref_cfg.sampling.proposal_field_2):
        c.grid.actor.use_4d_hashgrid = False
    refm = ref_cfg.setup(**kw()).eval()
    t.fill(hip)
    refm.load_state_dict(hip.state_dict())
    na = t.dense_nerfacc()
    ref_neurad.nerfacc = ref_renderers.nerfacc = na  # (restored by the `ref` fixture)
    refm._render_weights = lambda outputs, rs: na.render_weight_from_alpha(
        outputs[ref_neurad.FieldHeadNames.ALPHA].squeeze(-1))[0]
    return hip, refm


def _scan():
    from nerfstudio.cameras.lidars import Lidars, LidarType

    p = np.concatenate([synth.normal((PTS, 3), 44) * np.array([15.0, 15.0, 1.0], np.float32),
                        synth.uniform((PTS, 1), 0, 1, 46), synth.uniform((PTS, 1), -0.05, 0.05, 48)], -1).astype(np.float32)
    p[::10, :3] *= 200.0  # beyond the lidar's valid range: no return
    lidar = Lidars(lidar_to_worlds=T(t.poses(1, 40)), lidar_type=LidarType.VELODYNE64E, assume_ego_compensated=True,
                   times=T(synth.uniform((1, 1), 0.3, 3.5, 41)),
                   metadata={"velocities": T(synth.normal((1, 3), 42) * 3), "sensor_idxs": torch.full((1, 1), 2)},
                   valid_lidar_distance_threshold=1000.0)
    return T(p), lidar


def test_plugin_lidar_eval_glue_matches_the_reference_methods(ref, monkeypatch):  # noqa: F811
    hip, refm = _pair(ref)
    hip.config.eval_num_rays_per_chunk = refm.config.eval_num_rays_per_chunk = 40  # three chunks
    dev = DeviceStandIns().install(monkeypatch)
    points, lidar = _scan()
    # half of the rays predicted to return: the head's ray-drop bias at the median logit, on both models
    probe, _ = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    name = [k for k in hip.state_dict() if k.startswith("lidar_decoder") and k.endswith("bias")][-1]
    with torch.no_grad():
        for m in (hip, refm):
            dict(m.named_parameters())[name][1] -= float(probe["ray_drop_logits"].median())
    dev.calls.clear()
    got, gb = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    want, wb = refm.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    # device rays, three fused chunks, the whole scan through the lidar head in one call
    assert [c[0] for c in dev.calls] == ["lidar_rays"] + ["proposal_sampler_fwd", "render_fwd"] * 3 + ["mlp_fwd"]
    assert dev.calls[-1] == ("mlp_fwd", (PTS, 48))
    assert set(want) - set(got) == {"rgb"} and set(got) <= set(want)  # (the reference: an empty "rgb" for a scan)
    for k in sorted(set(got) - {"features"}):
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert rel_l2(N(got[k]), N(want[k])) < 2e-4, (k, rel_l2(N(got[k]), N(want[k])))
    assert set(gb) == set(wb) and gb["lidar_idx"] == 0
    for k in ("is_lidar", "did_return", "distance", "lidar"):
        assert gb[k].dtype == wb[k].dtype and torch.equal(gb[k], wb[k]), k
    assert 0 < int(gb["did_return"].sum()) < PTS and 0 < int((got["ray_drop_logits"] < 0).sum()) < PTS

    transfers = []
    to_host = type(hip)._scalars_to_host
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: (transfers.append(tuple(v.shape)), to_host(v))[1]))
    loss = hip.config.loss
    for case, mult, non_return in (("ray_drop", loss.ray_drop_loss_mult, 150.0), ("distance", 0.0, 150.0), ("fallback", 0.0, 0.0)):
        for cfg in (hip.config.loss, refm.config.loss):
            monkeypatch.setattr(cfg, "ray_drop_loss_mult", mult)
            monkeypatch.setattr(cfg, "non_return_lidar_distance", non_return)
        dev.calls.clear()
        metrics, images = hip.get_image_metrics_and_images(got, dict(gb))
        reference, _ = refm.get_image_metrics_and_images(got, dict(gb))  # the reference's code on the SAME outputs
        restated = R.lidar_metrics(N(got["depth"]), N(got["intensity"]), N(got["ray_drop_logits"]), N(got["points"]),
                                   N(gb["lidar"]), N(gb["distance"]), gb["did_return"][:, 0].numpy(), mult, non_return)
        assert images == {} and tuple(metrics) == R.METRIC_KEYS and all(type(v) is float for v in metrics.values())
        assert dev.calls == [("chamfer_distance", (PTS, 3), (PTS, 5), 3, 5)]  # the scan's [N,5] rows go in as they are
        for k in R.METRIC_KEYS:
            if k == "ray_drop_accuracy":
                assert np.float32(metrics[k]) == np.float32(float(reference[k])) == np.float32(restated[k]), (case, k)
            else:
                assert abs(metrics[k] - float(reference[k])) <= 1e-4 * abs(float(reference[k])), (case, k, metrics[k], reference[k])
                assert abs(metrics[k] - restated[k]) <= 1e-4 * abs(restated[k]), (case, k, metrics[k], restated[k])
        if case == "fallback":
            assert isinstance(reference["chamfer_distance"], torch.Tensor)  # (what this path returns as a float)
    assert transfers == [(5,)] * 3


def test_flag_off_leaves_the_reference_methods_in_charge(ref, monkeypatch):  # noqa: F811
    from nerfstudio.models.ad_model import ADModel
    from nerfstudio.models.neurad import NeuRADModel

    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModel, NeuRADHipModelConfig

    assert NeuRADHipModelConfig().fused_lidar_eval is False
    hip, _ = _pair(ref)
    hip.config.fused_lidar_eval = False
    called = []
    monkeypatch.setattr(NeuRADHipModel, "_scalars_to_host", staticmethod(lambda v: called.append("fused")))
    monkeypatch.setattr(ADModel, "get_outputs_for_lidar", lambda self, lidar, batch: called.append("outputs") or ("o", "b"))
    monkeypatch.setattr(NeuRADModel, "get_image_metrics_and_images",
                        lambda self, outputs, batch: called.append(("metrics", sorted(batch))) or ({}, {}))
    assert hip.get_outputs_for_lidar(None, {}) == ("o", "b")
    assert hip.get_image_metrics_and_images({"depth": torch.zeros(3, 1)}, {"lidar": torch.zeros(3, 5)}) == ({}, {})
    assert called == ["outputs", ("metrics", ["lidar"])]  # the batch goes through untouched, lidar key included
