"""tests/golden/ray_grads_edges.npz: the reference's fp32 autograd of the position gradients at the exact edges of the
contraction and the feature rescale, where several subgradients are possible and torch picks one.

  E1  |u|_inf tied on two axes (same and opposite signs) or on all three, outside the unit cube.  torch's inf-norm
      backward splits dL/dm evenly over the tied axes (torch.linalg.norm(ord=inf), spatial_distortions.py:126-141).
  E2  |u|_inf == 1: a sample on the cube's face; mask = mag < 1 is false, clamp_min(1) passes the gradient.
  E3  2 scal_0 std' == 1 at level 0 on an E2 sample: clamp_min(1.0) in the rescale (neurad_encoding.py:302) passes the
      gradient at equality.  Powers of two throughout: static_scale 16, min_res 32, area t^2 dist == 1, so both
      pow(1, 1/3) and the kernels' cube root give exactly 1 and every primal value is exact.
  and control rays with none of these.

Ties are exact in fp32 because the tied coordinates come from bitwise-equal (or negated) origin and direction
components.  Two cases:
  static  the static encoding alone (a random linear functional of the rescaled features): grads w.r.t. origins and
          directions, as case (1) of make_golden_raygrads.py.
  actor   three stationary actors with identity or 90-degree-yaw poses at power-of-two translations, actor_scale 1;
          dyadic rays put box-frame samples on E1 ties and E2 faces.  The reference's own pair selection and box-frame
          transform (NeuRADHashEncoding._split_static_vs_actors) and actor contraction, then a random linear functional
          of the contracted (mean, std): grads w.r.t. actor positions, rotations_6d, origins and directions.
Build container only:  python oracle/make_golden_grad_edges.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import ref_import

ref_import.install()
import synth  # noqa: E402
from make_golden import T, no_actors, save  # noqa: E402
from nerfstudio.cameras.rays import RayBundle  # noqa: E402
from nerfstudio.field_components.neurad_encoding import (  # noqa: E402
    ActorSettings, NeuRADHashEncodingConfig, StaticSettings)
from nerfstudio.fields.neurad_field import NeuRADField, NeuRADFieldConfig  # noqa: E402
from nerfstudio.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig  # noqa: E402

f32 = np.float32
STATIC_SCALE = 16.0
S = 8


def static_rays():
    """-> o, d [R,3], area [R], starts, ends [R,S], kind [R] (0 control, 1 E1, 2 E2, 3 E3 + E2)"""
    o, d, area, st, kind = [], [], [], [], []
    far = np.array([24, 40, 56, 72, 96, 128, 192, 256, 384], f32)  # bins past |u| = 1 for |d| >= 0.5
    face = np.array([4, 8, 12, 15.5, 16.5, 20, 40, 80, 160], f32)  # sample 3 at t = 16 exactly (dist 1/2)
    n = 0
    # E1: tied coordinates, origin 0 or with bitwise-equal / negated components
    for sgn in ((1, 1, 0), (1, -1, 0), (1, 0, 1), (0, -1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, -1)):
        for j in range(6):
            a = synth.uniform((1,), 0.5, 1.0, 1000 + n)[0]
            free = synth.uniform((3,), -0.45, 0.45, 1100 + n) * a
            dd = np.array([a * s if s else free[c] for c, s in enumerate(sgn)], f32)
            c0 = synth.uniform((1,), -3.0, 3.0, 1200 + n)[0] if j % 2 else f32(0)
            oo = np.array([c0 * s if s else free[c] for c, s in enumerate(sgn)], f32)
            o.append(oo), d.append(dd), area.append(synth.uniform((1,), 1e-7, 1e-5, 1300 + n)[0]), st.append(far)
            kind.append(1)
            n += 1
    # E2: one coordinate of the t = 16 sample on the face, some of them tied there too
    for sgn in ((1, 0, 0), (0, -1, 0), (0, 0, 1), (1, -1, 0), (-1, -1, -1)):
        for j in range(6):
            free = synth.uniform((3,), -0.9, 0.9, 1400 + n)
            dd = np.array([f32(s) if s else free[c] for c, s in enumerate(sgn)], f32)
            o.append(np.zeros(3, f32)), d.append(dd), area.append(synth.uniform((1,), 1e-7, 1e-5, 1500 + n)[0])
            st.append(face), kind.append(2)
            n += 1
    # E3: as E2 with area t^2 dist = 2^-7 * 256 * 1/2 = 1 -> std 1, std' = 1/64, 2 * 32 * std' = 1 at level 0
    for sgn in ((1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 1, 0), (-1, 1, 1)):
        for j in range(6):
            free = synth.uniform((3,), -0.9, 0.9, 1600 + n)
            dd = np.array([f32(s) if s else free[c] for c, s in enumerate(sgn)], f32)
            o.append(np.zeros(3, f32)), d.append(dd), area.append(f32(2.0 ** -7)), st.append(face), kind.append(3)
            n += 1
    # controls
    ro, rd, ra, _ = synth.rays(48, 1700)
    for i in range(48):
        o.append(ro[i]), d.append(rd[i]), area.append(ra[i] * (1 + i)), st.append(far * f32(0.5 + i / 32)), kind.append(0)
    bins = np.stack(st).astype(f32)
    return (np.stack(o).astype(f32), np.stack(d).astype(f32), np.array(area, f32), bins[:, :-1].copy(),
            bins[:, 1:].copy(), np.array(kind, np.int32))


def trajectories():
    """stationary actors (the same pose at every timestamp, so any interpolation weight gives the pose exactly)"""
    yaw90 = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out = []
    for rot, tr, dims in ((torch.eye(3), (32.0, 8.0, 0.0), (8.0, 4.0, 4.0)), (yaw90, (-16.0, 32.0, 1.0), (4.0, 8.0, 4.0)),
                          (torch.eye(3), (64.0, -32.0, 0.5), (4.0, 4.0, 4.0))):
        p = torch.eye(4)
        p[:3, :3] = rot
        p[:3, 3] = torch.tensor(tr)
        ts = torch.tensor([0.0, 1.0, 2.0])
        out.append({"timestamps": ts, "poses": p[None].repeat(3, 1, 1), "dims": torch.tensor(dims),
                    "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})
    return out


def actor_rays():
    """dyadic rays through the boxes; box-frame coordinates t/2 - 8 along tied axes, t = 8 .. 23: faces at t = 14, 18"""
    o, d = [], []
    # actor 0 (identity, at (32, 8, 0)): box frame = world - (32, 8, 0)
    for oo, dd in (((24, 0, 0), (0.5, 0.5, 0.0625)), ((24, 16, 0), (0.5, -0.5, 0.0625)), ((24, 0, -8), (0.5, 0.5, 0.5)),
                   ((24, 16, 8), (0.5, -0.5, -0.5)), ((24, 8.25, 0.5), (0.5, 0.0, 0.0))):
        o.append(oo), d.append(dd)
    # actor 1 (yaw 90 at (-16, 32, 1)): box frame = (y - 32, -(x + 16), z - 1)
    for oo, dd in (((-24, 24, 1), (0.5, 0.5, 0.0625)), ((-8, 24, 1), (-0.5, 0.5, 0.0)), ((-24, 24, -7), (0.5, 0.5, 0.5))):
        o.append(oo), d.append(dd)
    # actor 2 (identity at (64, -32, 0.5))
    for oo, dd in (((56, -40, 0.5), (0.5, 0.5, 0.0)), ((56, -24, -7.5), (0.5, -0.5, 0.5))):
        o.append(oo), d.append(dd)
    o, d = np.array(o, f32), np.array(d, f32)
    R = o.shape[0]
    st = np.broadcast_to(np.arange(7.5, 23.5, dtype=f32), (R, 16)).copy()
    return o, d, np.full((R,), 2.0 ** -12, f32), st, st + f32(1), np.array([0.0, 1.0, 2.0, 0.5, 1.5, 0.0, 2.0, 1.0,
                                                                           0.0, 2.0], f32)[:R]


def main():
    torch.manual_seed(0)
    kw = {}
    # ---- static ---------------------------------------------------------------------------------------------------
    grid = NeuRADHashEncodingConfig(static=StaticSettings(log2_hashmap_size=11))
    fld = NeuRADField(NeuRADFieldConfig(grid=grid, use_sdf=True), actors=no_actors(), static_scale=STATIC_SCALE,
                      implementation="torch").eval()
    fld.hashgrid.static_grid.hash_table.data = T(synth.hash_table(8 * 2**11, 4, seed=61, scale=0.5))
    o, d, area, starts, ends, kind = static_rays()
    R = o.shape[0]
    ot, dt = T(o).requires_grad_(True), T(d).requires_grad_(True)
    rb = RayBundle(origins=ot, directions=dt, pixel_area=T(area)[:, None], times=torch.zeros(R, 1),
                   nears=torch.zeros(R, 1), fars=torch.full((R, 1), 1000.0))
    rs = rb.get_ray_samples(T(starts)[..., None], T(ends)[..., None])
    feats, _ = fld.hashgrid(rs.frustums.get_fast_isotropic_gaussian(1), rs.times, rs.frustums.directions)
    g_enc = T(synth.normal(tuple(feats.shape), seed=181))
    (feats * g_enc).sum().backward()
    # (g_enc itself is not stored: synth.normal((R * S, 32), seed=181) regenerates it bit for bit)
    kw.update(o=o, d=d, area=area, starts=starts, ends=ends, kind=kind, enc_go=ot.grad, enc_gd=dt.grad,
              static_scale=np.array(STATIC_SCALE, f32))
    # ---- actor ----------------------------------------------------------------------------------------------------
    actors = DynamicActors(DynamicActorsConfig(), trajectories=trajectories())
    grid = NeuRADHashEncodingConfig(static=StaticSettings(log2_hashmap_size=11), require_actor_grad=True,
                                    actor=ActorSettings(actor_scale=1.0, log2_hashmap_size=9, use_4d_hashgrid=False))
    fld = NeuRADField(NeuRADFieldConfig(grid=grid), actors=actors, static_scale=100.0, implementation="torch").eval()
    actors.eval()
    o, d, area, starts, ends, times = actor_rays()
    R = o.shape[0]
    ot, dt = T(o).requires_grad_(True), T(d).requires_grad_(True)
    rb = RayBundle(origins=ot, directions=dt, pixel_area=T(area)[:, None], times=T(times)[:, None],
                   nears=torch.zeros(R, 1), fars=torch.full((R, 1), 60.0))
    rs = rb.get_ray_samples(T(starts)[..., None], T(ends)[..., None])
    hg = fld.hashgrid
    (ri, si, ai), apos, _ = hg._split_static_vs_actors(rs.frustums.get_fast_isotropic_gaussian(1), rs.times, None)
    cpos = hg.actor_contraction(apos)
    P = ri.shape[0]
    gx = T(synth.normal((P, 3), seed=191))
    gs = T(synth.normal((P,), seed=192))
    ((cpos.mean.reshape(P, 3) * gx).sum() + (cpos.std.reshape(P) * gs).sum()).backward()
    print("actor pairs:", P, "contracted:", int((apos.mean.reshape(P, 3).abs().amax(-1) >= 1).sum()))
    kw.update(a_o=o, a_d=d, a_area=area, a_starts=starts, a_ends=ends, a_times=times, a_ray=ri, a_sample=si, a_actor=ai,
              a_gx=gx, a_gs=gs, a_x01=cpos.mean.reshape(P, 3), a_cstd=cpos.std.reshape(P),
              a_timestamps=actors.unique_timestamps, a_positions=actors.actor_positions,
              a_rotations_6d=actors.actor_rotations_6d, a_present=actors.actor_present_at_time,
              a_bounds=actors.actor_bounds(), a_scale=np.array(1.0, f32),
              a_dpos=actors.actor_positions.grad, a_drot=actors.actor_rotations_6d.grad, a_go=ot.grad, a_gd=dt.grad)
    save("ray_grads_edges", **kw)


if __name__ == "__main__":
    main()
