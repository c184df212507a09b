"""CPU stand-ins for the device entry points a lidar scan's evaluation goes through in the plugin, for a host test of the
glue (tests/test_lidar_eval_plugin_host.py): the two fused eval kernels answered by the oracle (oracle/neurad_oracle.py),
the lidar head as torch linears, the ray generator by the reference's own ``Lidars.generate_rays`` and the chamfer op by
torch with direct differences.  Every call is recorded, so the test can check what reached the boundary."""
import numpy as np
import torch

import neurad_oracle as O
from plugin_harness import N_native as N
from plugin_harness import T


class DeviceStandIns:
    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        from neurad_studio_amd import ops
        from neurad_studio_amd.cameras import raygen

        for name in ("proposal_sampler_fwd", "render_fwd", "accumulate_along_rays", "mlp_fwd", "chamfer_distance"):
            monkeypatch.setattr(ops, name, getattr(self, name))
        monkeypatch.setattr(raygen, "lidar_rays", self.lidar_rays)
        return self

    @staticmethod
    def _grid(table, g):
        return O.GridParams(N(table), g.num_levels, g.min_res, g.max_res, g.log2_hashmap_size)

    def proposal_sampler_fwd(self, props, origins, directions, pixel_area, nears, fars, num_samples=(128, 64, 32), lam=-1.0,
                             scaling=0.1, histogram_padding=0.01, sky_distance=20000.0, actor_specs=None, cand=None):
        assert actor_specs is None and cand is None, "the stand-in covers the static scene"
        self.calls.append(("proposal_sampler_fwd", tuple(origins.shape), tuple(num_samples)))
        pp = [O.ProposalParams(self._grid(p.table, p.grid), p.static_scale, N(p.decoder_weight)) for p in props]
        R = origins.shape[0]
        so = O.proposal_sampler(pp, N(origins), N(directions), N(pixel_area).reshape(-1),
                                np.zeros(R, np.float32) if nears is None else N(nears).reshape(-1), N(fars).reshape(-1),
                                tuple(num_samples[:-1]), num_samples[-1], lam, scaling, sky_distance,
                                late_binding_quirk=False, stretch_sky=False)
        edges = lambda s, e: T(np.concatenate([s, e[:, -1:]], -1))  # noqa: E731
        sps = [T(b) for b in so.prop_spacing] + [edges(so.spacing_starts, so.spacing_ends)]
        eus = [edges(s, e) for s, e in zip(so.prop_starts, so.prop_ends)] + [edges(so.starts, so.ends)]
        return [T(w) for w in so.prop_weights], sps, eus

    def render_fwd(self, fs, origins, directions, pixel_area, starts, ends, return_weights=False, out=None,
                   early_stop_eps=0.0, order=None):
        self.calls.append(("render_fwd", tuple(origins.shape), tuple(starts.shape)))
        p = O.FieldParams(self._grid(fs.table, fs.grid), fs.static_scale, [N(w) for w in fs.geo_w], [N(b) for b in fs.geo_b],
                          [N(w) for w in fs.feat_w], [N(b) for b in fs.feat_b], beta=fs.beta, beta_min=0.0, use_sdf=fs.use_sdf)
        r = O.render_rays(p, N(origins), N(directions), N(pixel_area).reshape(-1), N(starts), N(ends))
        res = (T(r["features"]), T(r["depth"]).reshape(-1, 1), T(r["accumulation"]).reshape(-1, 1))
        return res + (T(r["weights"]),) if return_weights else res

    def accumulate_along_rays(self, weights, values=None):  # (the proposal rounds' depths; not recorded)
        return T(O.accumulate_along_rays(N(weights), None if values is None else N(values)))

    def mlp_fwd(self, x, weights, biases, save_hidden=False):
        """Linear (+ bias) + ReLU ... Linear; forward only"""
        self.calls.append(("mlp_fwd", tuple(x.shape)))
        for k, (w, b) in enumerate(zip(weights, biases)):
            x = torch.nn.functional.linear(x, w, b)
            x = x if k == len(weights) - 1 else torch.relu(x)
        return (x, None) if save_hidden else x

    def lidar_rays(self, lidars, lidar_indices, points, bundle_cls=None):
        self.calls.append(("lidar_rays", tuple(points.shape)))
        return lidars.generate_rays(lidar_indices=lidar_indices, points=points, keep_shape=True)

    def chamfer_distance(self, source, target, source_valid=None, target_valid=None, normalize_with_target=False,
                         return_per_point=False, plan=None):
        from neurad_studio_amd.model_components.lidar_metrics import nearest_sq_dist_torch

        self.calls.append(("chamfer_distance", tuple(source.shape), tuple(target.shape), source.stride(0), target.stride(0)))
        sv, tv = source_valid.bool(), target_valid.bool()
        total = (nearest_sq_dist_torch(source, target, sv, tv).double().sum()
                 + nearest_sq_dist_torch(target, source, tv, sv).double().sum())
        return (total / (tv.sum() if normalize_with_target else 1)).float()
