"""Golden vectors for the fused field kernels' small grids (L * F < 32), produced by the reference itself
(NeuRADField(implementation="torch")), the way oracle/make_golden.py's golden_field does:

  * tests/golden/field_tiny.npz         BASELINE config[0]'s field: a 1-level grid, 4 features, resolution 32,
                                        2^10 rows, 32-wide MLPs, SDF head.  Outputs + gradients through a random
                                        linear functional (sparse table gradient, all MLP gradients, dbeta).
  * tests/golden/field_neurad_tiny.npz  the "NeuRAD tiny" static grid: 4 levels x 2 features, 32-wide MLPs; same contents.
  * tests/golden/field_neurad_tiny_actors.npz  the same static grid with 3 dynamic actors whose grids have 2 levels x 2
                                        features: eval outputs (as oracle/make_golden_actors.py).

Inputs and weights come from tests/synth.py; the files hold only the inputs and the reference's outputs.  Run where the
reference tree is present:  python scripts/make_golden_field_shapes.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402

ref_import.install()
import synth  # noqa: E402
from make_golden import T, make_bundle, no_actors, save, set_linear  # noqa: E402
from make_golden_actors import trajectories  # noqa: E402
from nerfstudio.cameras.rays import RayBundle  # noqa: E402
from nerfstudio.field_components.field_heads import FieldHeadNames  # noqa: E402
from nerfstudio.field_components.neurad_encoding import ActorSettings, NeuRADHashEncodingConfig, StaticSettings  # noqa: E402
from nerfstudio.fields.neurad_field import NeuRADField, NeuRADFieldConfig  # noqa: E402
from nerfstudio.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig  # noqa: E402
from nerfstudio.model_components.ray_samplers import PowerSampler  # noqa: E402

# tag -> (static grid settings, table seed); the tests rebuild the tables from the same (rows, F, seed, scale)
SHAPES = {
    "tiny": (dict(hashgrid_dim=4, num_levels=1, base_res=32, max_res=32, log2_hashmap_size=10), 53),
    "neurad_tiny": (dict(hashgrid_dim=2, num_levels=4, log2_hashmap_size=11), 57),
}
R, S = 32, 40  # S: two full 16-sample tiles and a ragged third


def set_mlps(fld):
    for k, l in enumerate(fld.mlp_geo.layers):
        set_linear(l, 200 + 10 * k)
    for k, l in enumerate(fld.mlp_feature.layers):
        set_linear(l, 300 + 10 * k)


def golden_static(tag):
    st, seed = SHAPES[tag]
    L, F, lg = st["num_levels"], st["hashgrid_dim"], st["log2_hashmap_size"]
    grid = NeuRADHashEncodingConfig(static=StaticSettings(**st), require_actor_grad=True, actor=ActorSettings(flip_prob=0.25))
    fld = NeuRADField(NeuRADFieldConfig(grid=grid), actors=no_actors(), static_scale=100.0, implementation="torch").eval()
    fld.hashgrid.static_grid.hash_table.data = T(synth.hash_table(L * 2**lg, F, seed=seed, scale=0.5))
    set_mlps(fld)
    rb, (o, d, area, t) = make_bundle(R, seed=61)
    rs = PowerSampler(num_samples=S, lambda_=-1.0, scaling=0.1).eval()(rb)
    out = fld(rs)
    starts, ends = rs.frustums.starts[..., 0], rs.frustums.ends[..., 0]
    kw = dict(o=o, d=d, area=area, starts=starts, ends=ends, feature=out[FieldHeadNames.FEATURE],
              sdf=out[FieldHeadNames.SDF][..., 0], alpha=out[FieldHeadNames.ALPHA][..., 0])
    # gradients through a random linear functional of the outputs
    gf = T(synth.normal(tuple(out[FieldHeadNames.FEATURE].shape), seed=71))
    ga = T(synth.normal(tuple(out[FieldHeadNames.ALPHA].shape), seed=72))
    ((out[FieldHeadNames.FEATURE] * gf).sum() + (out[FieldHeadNames.ALPHA] * ga).sum()).backward()
    tg = fld.hashgrid.static_grid.hash_table.grad
    nz = tg.abs().sum(-1) > 0
    kw.update(g_feature=gf, g_head=ga[..., 0], tg_idx=nz.nonzero()[:, 0], tg_val=tg[nz], dbeta=fld.sdf_to_density.beta.grad,
              **{f"geo_dw{k}": l.weight.grad for k, l in enumerate(fld.mlp_geo.layers)},
              **{f"geo_db{k}": l.bias.grad for k, l in enumerate(fld.mlp_geo.layers)},
              **{f"feat_dw{k}": l.weight.grad for k, l in enumerate(fld.mlp_feature.layers)},
              **{f"feat_db{k}": l.bias.grad for k, l in enumerate(fld.mlp_feature.layers)})
    save(f"field_{tag}", **kw)


def golden_actors():
    st, seed = SHAPES["neurad_tiny"]
    actors = DynamicActors(DynamicActorsConfig(), trajectories=trajectories())
    grid = NeuRADHashEncodingConfig(static=StaticSettings(**st),
                                    actor=ActorSettings(flip_prob=0.25, hashgrid_dim=2, num_levels=2, log2_hashmap_size=9,
                                                        use_4d_hashgrid=False))
    fld = NeuRADField(NeuRADFieldConfig(grid=grid), actors=actors, static_scale=100.0, implementation="torch").eval()
    actors.eval()
    fld.hashgrid.static_grid.hash_table.data = T(synth.hash_table(4 * 2**11, 2, seed=seed, scale=0.5))
    for i, g in enumerate(fld.hashgrid.actor_grids):
        g.hash_table.data = T(synth.hash_table(2 * 2**9, 2, seed=400 + i, scale=0.7))
    set_mlps(fld)
    # rays from the origin region aimed at the actors' corridor (oracle/make_golden_actors.py)
    Ra, Sa = 48, 40
    o = synth.normal((Ra, 3), 7) * np.array([1.0, 1.0, 0.2], np.float32)
    tgt = np.stack([synth.uniform((Ra,), 10, 24, 8), np.where(np.arange(Ra) % 2 == 0, 8.0, -5.5)
                    + synth.uniform((Ra,), -1.5, 1.5, 9), synth.uniform((Ra,), 0.0, 1.0, 10)], -1).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d.astype(np.float32)
    times = synth.uniform((Ra,), -0.5, 4.5, 11)
    rb = RayBundle(origins=T(o), directions=T(d), pixel_area=torch.full((Ra, 1), 2.43e-6), times=T(times)[:, None],
                   nears=torch.zeros(Ra, 1), fars=torch.full((Ra, 1), 60.0))
    rs = PowerSampler(num_samples=Sa, lambda_=-1.0, scaling=0.1).eval()(rb)
    with torch.no_grad():
        out = fld(rs)
        gauss = rs.frustums.get_fast_isotropic_gaussian(1)
        feats, dirs = fld.hashgrid(gauss, rs.times, rs.frustums.directions)
        idx, _, _ = fld.hashgrid._split_static_vs_actors(gauss, rs.times, rs.frustums.directions)
    print("actor-hit samples:", idx[0].shape[0], "of", Ra * Sa)
    save("field_neurad_tiny_actors", o=o, d=d, area=np.full((Ra,), 2.43e-6, np.float32), times=times,
         starts=rs.frustums.starts[..., 0], ends=rs.frustums.ends[..., 0], feature=out[FieldHeadNames.FEATURE],
         sdf=out[FieldHeadNames.SDF][..., 0], alpha=out[FieldHeadNames.ALPHA][..., 0], enc=feats, directions=dirs,
         hit_ray=idx[0], hit_sample=idx[1], hit_actor=idx[2], timestamps=actors.unique_timestamps,
         positions=actors.actor_positions, rotations_6d=actors.actor_rotations_6d, present=actors.actor_present_at_time,
         sizes=actors.actor_sizes, padding=actors.actor_padding)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    golden_static("tiny")
    golden_static("neurad_tiny")
    golden_actors()
