"""Evaluation of a lidar scan through the plugin (``NeuRADHipModelConfig.fused_lidar_eval``) on the GPU against the reference
model on the CPU with the same weights (plugin_harness.build_pair): ``get_outputs_for_lidar`` (models/ad_model.py:85-114)
at the tolerance of the eval-output comparison of tests/test_gpu_reference_plugin.py, the lidar branch of
``get_image_metrics_and_images`` (models/neurad.py:589-620) against the float64 restatement (tests/lidar_eval_refs.py)
evaluated on the plugin's OWN outputs -- which separates the metric code from the render difference -- in its three cases,
one device->host transfer per scan, and the flag off leaving the reference's methods in charge."""
import os
import sys

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
from plugin_harness import N, T, ref  # noqa: E402,F401

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_import.reference_available(),
                                 reason="no reference: run `python oracle/make_ref.py` in the build container "
                                        "(oracle/_ref ships with the lease)")]
PTS = 2500


def scan_and_lidar():
    """one sweep of PTS beams around a lidar 1.6 m above the origin; every tenth beam ends beyond the lidar's valid range"""
    from nerfstudio.cameras.lidars import Lidars, LidarType

    p = np.concatenate([synth.normal((PTS, 3), 44) * np.array([15.0, 15.0, 1.0], np.float32),
                        synth.uniform((PTS, 1), 0, 1, 46), synth.uniform((PTS, 1), -0.05, 0.05, 48)], -1).astype(np.float32)
    p[::10, :3] *= 200.0
    lidar = Lidars(lidar_to_worlds=T(t.poses(1, 40)), lidar_type=LidarType.VELODYNE64E, assume_ego_compensated=True,
                   times=T(synth.uniform((1, 1), 0.3, 3.5, 41)),
                   metadata={"velocities": T(synth.normal((1, 3), 42) * 3), "sensor_idxs": torch.full((1, 1), 2)},
                   valid_lidar_distance_threshold=1000.0)
    return T(p), lidar


@pytest.fixture(scope="module")
def rendered(ref):  # noqa: F811
    """the pair, the plugin's outputs for the scan with the flag on, the reference's on the CPU (computed once, shared)"""
    hip, refm = t.build_pair(ref, False)
    t.deterministic(hip, False), t.deterministic(refm, False)
    hip.config.fused_lidar_eval = True
    hip.config.eval_num_rays_per_chunk = refm.config.eval_num_rays_per_chunk = 1024  # three chunks
    points, lidar = scan_and_lidar()
    # the synthetic weights give every ray a positive ray-drop logit: shift the head's bias (both models) to the median logit,
    # so that half of the rays are predicted to return
    probe, _ = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    shift = float(probe["ray_drop_logits"].median())
    name = [k for k in hip.state_dict() if k.startswith("lidar_decoder") and k.endswith("bias")][-1]
    with torch.no_grad():
        for m in (hip, refm):
            bias = dict(m.named_parameters())[name]
            assert bias.shape == (2,)
            bias[1] -= shift
    got, got_batch = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    want, want_batch = refm.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    return hip, refm, got, got_batch, want, want_batch


def test_outputs_for_lidar_match_the_reference(rendered):
    hip, refm, got, got_batch, want, want_batch = rendered
    assert set(want) - set(got) <= {"rgb"}  # (the reference: an empty tensor for a scan)
    for k in ("points", "depth", "intensity", "ray_drop_logits"):
        assert got[k].shape == want[k].shape and got[k].is_cuda, (k, got[k].shape, want[k].shape)
        assert rel_l2(N(got[k]), N(want[k])) < 1e-4, (k, rel_l2(N(got[k]), N(want[k])))
    for k in ("is_lidar", "did_return", "distance"):
        assert got_batch[k].shape == want_batch[k].shape and got_batch[k].is_cuda, k
    assert torch.equal(got_batch["did_return"].cpu(), want_batch["did_return"]) and bool(got_batch["is_lidar"].all())
    assert 0 < int(got_batch["did_return"].sum()) < PTS
    assert rel_l2(N(got_batch["distance"]), N(want_batch["distance"])) < 1e-6


def _restated(hip, out, batch, mult, non_return=R.NON_RETURN_DISTANCE):
    return R.lidar_metrics(N(out["depth"]), N(out["intensity"]), N(out["ray_drop_logits"]), N(out["points"]),
                           N(batch["lidar"]), N(batch["distance"]), batch["did_return"][:, 0].cpu().numpy(), mult, non_return)


def _check(got, want, case):
    assert set(got) == set(R.METRIC_KEYS) and all(type(v) is float for v in got.values()), got
    for k in R.METRIC_KEYS:
        if k == "ray_drop_accuracy":
            assert np.float32(got[k]) == np.float32(want[k]), (case, k, got[k], want[k])
        else:
            assert abs(got[k] - want[k]) <= 1e-4 * abs(want[k]), (case, k, got[k], want[k])


def test_lidar_metrics_match_the_restatement_on_the_plugins_own_outputs(rendered, monkeypatch):
    hip, refm, out, batch, _, _ = rendered
    transfers = []
    to_host = type(hip)._scalars_to_host
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: (transfers.append(tuple(v.shape)), to_host(v))[1]))
    loss = hip.config.loss
    assert loss.ray_drop_loss_mult > 0 and loss.non_return_lidar_distance == R.NON_RETURN_DISTANCE
    got, images = hip.get_image_metrics_and_images(out, dict(batch))
    assert images == {} and transfers == [(5,)]  # the five scalars, one transfer
    want = _restated(hip, out, batch, loss.ray_drop_loss_mult)
    _check(got, want, "ray_drop")
    assert bool((out["ray_drop_logits"] < 0).any()) and bool(batch["did_return"].any())  # (not the fallback)
    # returns predicted by distance
    monkeypatch.setattr(loss, "ray_drop_loss_mult", 0.0)
    got0, _ = hip.get_image_metrics_and_images(out, dict(batch))
    _check(got0, _restated(hip, out, batch, 0.0), "distance")
    assert got0["chamfer_distance"] != got["chamfer_distance"] and len(transfers) == 2
    # the fallback (models/neurad.py:619-620): no ray predicted to return -> the mean range of the returned points, a float
    monkeypatch.setattr(loss, "non_return_lidar_distance", 0.0)
    got_fb, _ = hip.get_image_metrics_and_images(out, dict(batch))
    want_fb = _restated(hip, out, batch, 0.0, 0.0)
    ret = batch["did_return"][:, 0].cpu().numpy()
    assert want_fb["chamfer_distance"] == np.linalg.norm(N(batch["lidar"]).astype(np.float64)[ret, :3], axis=-1).mean()
    _check(got_fb, want_fb, "fallback")
    assert len(transfers) == 3


def test_flag_off_leaves_the_reference_methods_in_charge(rendered, monkeypatch):
    hip, refm, out, batch, _, _ = rendered
    from nerfstudio.models.ad_model import ADModel
    from nerfstudio.models.neurad import NeuRADModel

    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModelConfig

    assert NeuRADHipModelConfig().fused_lidar_eval is False
    monkeypatch.setattr(hip.config, "fused_lidar_eval", False)
    called = []
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: called.append("fused")))
    monkeypatch.setattr(ADModel, "get_outputs_for_lidar", lambda self, lidar, batch: called.append("reference") or ("o", "b"))
    assert hip.get_outputs_for_lidar(None, {}) == ("o", "b") and called == ["reference"]
    got, _ = hip.get_image_metrics_and_images(out, dict(batch))
    want, _ = NeuRADModel.get_image_metrics_and_images(hip, out, dict(batch))
    assert called == ["reference"] and set(got) == set(want) == set(R.METRIC_KEYS)
    assert all(float(got[k]) == float(want[k]) for k in got)
