"""The plugin's ``median_depth`` flag on the CPU, with stand-ins for the device (tests/lidar_eval_standins.py plus the two
median-depth ops answered by the restatement, tests/median_depth_refs.py), in the manner of
tests/test_lidar_eval_plugin_host.py: with ``fused_lidar_eval`` a scan's outputs gain ``median_depth`` and ``median_points``,
its metrics the three keys of LIDAR_EVAL_MEDIAN_KEYS -- the five-metric code applied to the median depth and its points --
and all eight scalars leave in ONE transfer; with the flag off the outputs, the five keys and the transfer of shape (5,) are
what they were.  The kernels themselves are tested on the GPU (tests/test_gpu_median_depth.py)."""
import os
import sys
from copy import deepcopy

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lidar_eval_refs as R  # noqa: E402
import median_depth_refs as M  # noqa: E402
import plugin_harness as t  # noqa: E402
import ref_import  # noqa: E402
import synth  # noqa: E402
from lidar_eval_standins import DeviceStandIns  # noqa: E402
from plugin_harness import N, T, ref  # noqa: E402,F401

pytestmark = pytest.mark.skipif(not ref_import.reference_available(), reason="no reference tree")
PTS = 96
MEDIAN_KEYS = ("median_depth_median_l2", "median_depth_mean_rel_l2", "median_chamfer_distance")


def _model(median_depth):
    from nerfstudio.data.scene_box import SceneBox

    mcfg = t.shrink(deepcopy(t.methods()["neurad-hip"].pipeline.model))
    mcfg.fused_decoder, mcfg.fused_lidar_eval, mcfg.median_depth = False, True, median_depth
    torch.manual_seed(0)
    hip = mcfg.setup(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                     metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"},
                               "trajectories": []}).eval()
    t.fill(hip)
    hip.config.eval_num_rays_per_chunk = 40  # three chunks
    return hip


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


class MedianStandIns(DeviceStandIns):
    """... plus the two median-depth ops from the restatement; the render stand-in's weights and the rays are kept"""

    def __init__(self):
        super().__init__()
        self.rendered, self.bundles = [], []

    def install(self, monkeypatch):
        from neurad_studio_amd import ops

        super().install(monkeypatch)
        monkeypatch.setattr(ops, "median_depth", self.median_depth)
        monkeypatch.setattr(ops, "median_depth_packed", self.median_depth_packed)
        return self

    def render_fwd(self, fs, origins, directions, pixel_area, starts, ends, return_weights=False, **kw):
        out = super().render_fwd(fs, origins, directions, pixel_area, starts, ends, return_weights, **kw)
        self.rendered.append((return_weights, out[3] if return_weights else None, starts, ends))
        return out

    def lidar_rays(self, lidars, lidar_indices, points, bundle_cls=None):
        self.bundles.append(super().lidar_rays(lidars, lidar_indices, points, bundle_cls))
        return self.bundles[-1]

    def median_depth(self, weights, starts, ends, thresholds=(0.5,), return_index=False):
        self.calls.append(("median_depth", tuple(weights.shape)))
        d, i = M.median_depth(weights.numpy(), starts.numpy(), ends.numpy(), thresholds)
        return (T(d), torch.from_numpy(i)) if return_index else T(d)

    def median_depth_packed(self, weights, t_starts, t_ends, segments, thresholds=(0.5,), return_index=False):
        self.calls.append(("median_depth_packed", tuple(weights.shape)))
        d, i = M.median_depth_packed(weights.numpy(), t_starts.numpy(), t_ends.numpy(), segments.numpy(), thresholds)
        return (T(d), torch.from_numpy(i)) if return_index else T(d)


def _shift_ray_drop_bias(hip, lidar, points):
    """half of the rays predicted to return: the head's ray-drop bias at the median logit"""
    probe, _ = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    name = [k for k in hip.state_dict() if k.startswith("lidar_decoder") and k.endswith("bias")][-1]
    with torch.no_grad():
        dict(hip.named_parameters())[name][1] -= float(probe["ray_drop_logits"].median())


def test_median_depth_outputs_and_eight_metrics_in_one_transfer(ref, monkeypatch):  # noqa: F811
    from nerfstudio.utils.poses import inverse as pose_inverse

    from neurad_studio_amd.integration.neurad_hip import NeuRADHipModelConfig
    from neurad_studio_amd.model_components import lidar_metrics as LM

    assert NeuRADHipModelConfig().median_depth is False and LM.LIDAR_EVAL_MEDIAN_KEYS == MEDIAN_KEYS
    assert LM.LIDAR_EVAL_KEYS == R.METRIC_KEYS
    hip = _model(True)
    assert hip.median_depth is True
    dev = MedianStandIns().install(monkeypatch)
    points, lidar = _scan()
    _shift_ray_drop_bias(hip, lidar, points)
    dev.calls.clear(), dev.rendered.clear(), dev.bundles.clear()
    got, gb = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    S = dev.rendered[0][2].shape[1]
    assert [c[0] for c in dev.calls] == ["lidar_rays"] + ["proposal_sampler_fwd", "render_fwd", "median_depth"] * 3 + ["mlp_fwd"]
    assert [c for c in dev.calls if c[0] == "median_depth"] == [("median_depth", (40, S - 1)), ("median_depth", (40, S - 1)),
                                                                ("median_depth", (16, S - 1))]
    assert all(r[0] for r in dev.rendered)  # the weights were asked for
    assert {"median_depth", "median_points", "depth", "points"} <= set(got)
    assert got["median_depth"].shape == got["depth"].shape == (PTS, 1) and got["median_points"].shape == got["points"].shape
    # the median of the non-sky samples of the very weights the render handed out
    w, s, e = (torch.cat([r[k] for r in dev.rendered]).numpy()[:, :-1] for k in (1, 2, 3))
    want, idx = M.median_depth(w, s, e)
    assert np.array_equal(N(got["median_depth"]), want) and len(set(idx[:, 0].tolist())) > 3
    assert not np.array_equal(N(got["median_depth"]), N(got["depth"]))
    # median_points: built like points (models/ad_model.py:108-113) from the median depth
    rb = dev.bundles[0]
    for pk, dk in (("points", "depth"), ("median_points", "median_depth")):
        world = rb.origins + rb.directions * got[dk]
        expect = (pose_inverse(lidar.lidar_to_worlds[0]) @ torch.cat([world, torch.ones_like(world[..., :1])], -1).unsqueeze(-1))
        assert torch.equal(got[pk], expect.squeeze(-1)), pk

    transfers = []
    to_host = type(hip)._scalars_to_host
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: (transfers.append(tuple(v.shape)), to_host(v))[1]))
    loss = hip.config.loss
    as_median = {**{k: v for k, v in got.items() if not k.startswith("median_")}, "depth": got["median_depth"],
                 "points": got["median_points"]}
    plain = {k: v for k, v in got.items() if not k.startswith("median_")}
    for case, mult, non_return in (("ray_drop", loss.ray_drop_loss_mult, 150.0), ("distance", 0.0, 150.0), ("fallback", 0.0, 0.0)):
        monkeypatch.setattr(loss, "ray_drop_loss_mult", mult)
        monkeypatch.setattr(loss, "non_return_lidar_distance", non_return)
        dev.calls.clear()
        metrics, images = hip.get_image_metrics_and_images(got, dict(gb))
        assert images == {} and tuple(metrics) == R.METRIC_KEYS + MEDIAN_KEYS and all(type(v) is float for v in metrics.values())
        assert [c[0] for c in dev.calls] == ["chamfer_distance"] * 2
        assert len(transfers) == 1 and transfers.pop() == (8,)  # all eight, one transfer
        # the five: what the flag-off code gives on the same outputs; the three: that code on the median depth and points
        five = LM.lidar_eval_metrics(plain, points, gb["distance"], gb["did_return"][:, 0], mult, non_return)
        on_median = LM.lidar_eval_metrics(as_median, points, gb["distance"], gb["did_return"][:, 0], mult, non_return)
        assert tuple(five) == tuple(on_median) == R.METRIC_KEYS
        assert {k: metrics[k] for k in R.METRIC_KEYS} == five, case
        for mk, k in zip(MEDIAN_KEYS, ("depth_median_l2", "depth_mean_rel_l2", "chamfer_distance")):
            assert metrics[mk] == on_median[k], (case, mk)
        restated = R.lidar_metrics(N(got["median_depth"]), N(got["intensity"]), N(got["ray_drop_logits"]),
                                   N(got["median_points"]), N(gb["lidar"]), N(gb["distance"]), gb["did_return"][:, 0].numpy(),
                                   mult, non_return)
        for mk, k in zip(MEDIAN_KEYS, ("depth_median_l2", "depth_mean_rel_l2", "chamfer_distance")):
            assert abs(metrics[mk] - restated[k]) <= 1e-4 * abs(restated[k]), (case, mk, metrics[mk], restated[k])
        if case != "fallback":
            assert metrics["median_chamfer_distance"] != metrics["chamfer_distance"]
        else:
            assert metrics["median_chamfer_distance"] == metrics["chamfer_distance"]  # the mean range of the returns


def test_flag_off_changes_nothing(ref, monkeypatch):  # noqa: F811
    hip = _model(False)
    assert hip.median_depth is False
    dev = MedianStandIns().install(monkeypatch)
    points, lidar = _scan()
    _shift_ray_drop_bias(hip, lidar, points)
    dev.calls.clear(), dev.rendered.clear()
    got, gb = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    assert [c[0] for c in dev.calls] == ["lidar_rays"] + ["proposal_sampler_fwd", "render_fwd"] * 3 + ["mlp_fwd"]
    assert not any(r[0] for r in dev.rendered)  # no weights asked for
    assert not any(k.startswith("median") for k in got)
    transfers = []
    to_host = type(hip)._scalars_to_host
    monkeypatch.setattr(type(hip), "_scalars_to_host", staticmethod(lambda v: (transfers.append(tuple(v.shape)), to_host(v))[1]))
    dev.calls.clear()
    metrics, images = hip.get_image_metrics_and_images(got, dict(gb))
    assert images == {} and tuple(metrics) == R.METRIC_KEYS and transfers == [(5,)]
    assert [c[0] for c in dev.calls] == ["chamfer_distance"]
    # the same model with the flag on: the outputs it shares are the same tensors' values, the five metrics the same floats
    hip.median_depth = True
    got_on, gb_on = hip.get_outputs_for_lidar(lidar, {"lidar": points.clone(), "lidar_idx": 0})
    assert set(got_on) == set(got) | {"median_depth", "median_points"}
    for k in got:
        assert torch.equal(got_on[k], got[k]), k
    metrics_on, _ = hip.get_image_metrics_and_images(got_on, dict(gb_on))
    assert transfers == [(5,), (8,)] and {k: metrics_on[k] for k in R.METRIC_KEYS} == metrics
