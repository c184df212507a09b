"""CPU stand-ins for the ``ops`` entry points one fused TRAINING step of the plugin calls on a static scene, answered by the
oracle (oracle/neurad_oracle.py) -- forward only: the fused nodes' backward passes are kernels.  A helper module (test modules
are not libraries: tests/test_helper_layout.py); tests/test_reference_integration.py keeps stand-ins of its own for the eval
path.  Used by tests/test_camera_opt_plugin_host.py.  The lidar head's MLP and the distortion / interlevel losses are not ops of
the fused nodes: ``install`` answers the first with torch and leaves the other two to the caller."""
import numpy as np
import torch

import neurad_oracle as O
from plugin_harness import N_native as N
from plugin_harness import T

NAMES = ("power_sampler", "proposal_density_fwd", "prop_weights_fwd", "pdf_sample", "field_fwd_train", "sdf_render_fwd",
         "appearance_fwd", "lidar_carving", "mlp_fwd")


class TrainStepStandIns:
    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        from neurad_studio_amd import ops

        for name in NAMES:
            monkeypatch.setattr(ops, name, getattr(self, name))
        return self

    @staticmethod
    def _grid(table, g):
        return O.GridParams(N(table), g.num_levels, g.min_res, g.max_res, g.log2_hashmap_size)

    def power_sampler(self, nears, fars, num_samples, lam=-1.0, scaling=0.1, t_rand=None, last_edge=0.0):
        self.calls.append("power_sampler")
        n = np.zeros(fars.numel(), np.float32) if nears is None else N(nears).reshape(-1)
        bins, eu, _ = O.power_sampler(n, N(fars).reshape(-1), num_samples, lam, scaling, None if t_rand is None else N(t_rand))
        return T(bins), T(eu)

    def proposal_density_fwd(self, ps, origins, directions, pixel_area, starts, ends, save_features=False):
        self.calls.append("proposal_density_fwd")
        p = O.ProposalParams(self._grid(ps.table, ps.grid), ps.static_scale, N(ps.decoder_weight))
        dens = T(O.proposal_density(p, N(origins), N(directions), N(pixel_area), N(starts), N(ends)))
        return (dens, torch.zeros(ps.grid.num_levels, dens.numel())) if save_features else dens

    def prop_weights_fwd(self, edges, densities, want_depth=True):
        self.calls.append("prop_weights_fwd")
        e, dn = N(edges), N(densities)
        w = O.weights_from_density(e[:, 1:] - e[:, :-1], dn)
        return T(w), T((w * (e[:, 1:] + e[:, :-1]) / 2).sum(-1, keepdims=True).astype(np.float32))

    def pdf_sample(self, weights, spacing_bins, nears, fars, num_samples, lam=-1.0, scaling=0.1, histogram_padding=0.01,
                   rand=None):
        self.calls.append("pdf_sample")
        R = weights.shape[0]
        n = np.zeros((R, 1), np.float32) if nears is None else N(nears).reshape(-1, 1)
        f = N(fars).reshape(-1, 1)
        sp = O.Spacing(O.power_fn(n * np.float32(scaling), lam), O.power_fn(f * np.float32(scaling), lam), lam, scaling)
        bins, eu = O.pdf_sample(N(weights), N(spacing_bins), num_samples, sp, histogram_padding,
                                rand=None if rand is None else N(rand).reshape(R, -1))
        return T(bins), T(eu)

    def field_fwd_train(self, fs, origins, directions, pixel_area, starts, ends, order=None, override=None):
        assert override is None, "static scenes only"
        self.calls.append("field_fwd_train")
        p = O.FieldParams(self._grid(fs.table, fs.grid), fs.static_scale, [N(w) for w in fs.geo_w], [N(b) for b in fs.geo_b],
                          [N(w) for w in fs.feat_w], [N(b) for b in fs.feat_b], beta=fs.beta, beta_min=0.0, use_sdf=fs.use_sdf)
        out = O.field_fwd(p, N(origins), N(directions), N(pixel_area), N(starts), N(ends))
        n = starts.shape[0] * starts.shape[1]
        z = torch.zeros(n, 1)
        return (T(out["feature"]).reshape(n, -1), T(out["sdf"]).reshape(n), z[:, 0]), (z, z, z, z)

    def sdf_render_fwd(self, sdf, beta, beta_min, features, edges, extra_cols=0):
        self.calls.append("sdf_render_fwd")
        e = N(edges)
        alpha = O.sigmoid(-N(sdf) * np.float32(abs(float(beta)) + beta_min))
        w, _ = O.render_weight_from_alpha(alpha)
        feats, depth, acc = O.composite(w, N(features), e[:, :-1], e[:, 1:])
        out = torch.zeros(sdf.shape[0], feats.shape[1] + extra_cols)
        out[:, :feats.shape[1]] = T(feats)
        return T(alpha), T(w[:, :-1].copy()), out, T(depth).reshape(-1, 1), T(acc).reshape(-1, 1)

    def appearance_fwd(self, weight, sensor_idx, times, duration, n_per_sensor, temporal, n_rays, out=None):
        self.calls.append("appearance_fwd")
        wt = N(weight)
        s = np.zeros(n_rays, np.int64) if sensor_idx is None else N(sensor_idx).reshape(-1)
        if temporal and times is not None:
            ti = N(times).reshape(-1) / np.float32(duration) * np.float32(n_per_sensor)
            lo = np.clip(np.floor(ti), 0, n_per_sensor - 1)
            hi = np.clip(lo + 1, 0, n_per_sensor - 1)
            fr = (ti - lo)[:, None].astype(np.float32)
            val = wt[(lo + s * n_per_sensor).astype(np.int64)] * (1 - fr) + wt[(hi + s * n_per_sensor).astype(np.int64)] * fr
        else:
            val = wt[s]
        out.copy_(T(val.astype(np.float32)))
        return out

    def lidar_carving(self, starts, ends, is_lidar, did_return, distance, carving_epsilon, non_return_lidar_distance,
                      weights=None, want_mask=True, want_grad=True):
        self.calls.append("lidar_carving")
        mid = (N(starts) + N(ends)) * 0.5
        lid = N(is_lidar).reshape(-1, 1).astype(bool)
        close_hit = np.abs(N(distance).reshape(-1, 1) - mid) < carving_epsilon
        if did_return is None:
            close = lid & close_hit
        else:
            ret = N(did_return).reshape(-1, 1).astype(bool)
            close = lid & ((ret & close_hit) | (~ret & (mid < non_return_lidar_distance)))
        loss = gw = None
        if weights is not None:
            m = (lid & ~close).astype(np.float32)
            loss = T(((N(weights) * m) ** 2).sum(-1).astype(np.float32))
            gw = T((2 * N(weights) * m).astype(np.float32))
        return (torch.from_numpy(close) if want_mask else None), loss, gw

    def mlp_fwd(self, x, weights, biases, save_hidden=False):
        h, hidden = x, []
        for i, (w, b) in enumerate(zip(weights, biases)):
            h = torch.nn.functional.linear(h, w, b)
            if i < len(weights) - 1:
                h = torch.relu(h)
                hidden.append(h)
        return (h, torch.cat(hidden, 1) if hidden else None) if save_hidden else h
