"""What the tests of the occupancy route with dynamic actors share (tests/test_render_packed_actors_host.py,
tests/test_gpu_packed_actors.py): the two scenes, the fields of the five actor shapes, the
numpy restatement of the box-aware march rule, and the references of the fused packed render with actors.

The march rule (csrc/occgrid.hip): the candidate intervals are those of the plain march; one is kept iff its level's cell is
set OR its sample position -- the mean the field evaluates, o + d (t0 + (t1 - t0) / 2) -- lies strictly inside the box of
one of the actors present at the ray's time."""
import functools

import numpy as np
import torch

import neurad_oracle as O
import occgrid_oracle as OO
import occgrid_update_restatement as OU
import packed_restatement as PR
import synth
from builders import field_params, trajectories
from conftest import load_golden, rel_l2

f32 = np.float32
SHAPES = ((8, 4, 32), (8, 4, 64), (16, 2, 64), (4, 2, 32), (4, 2, 64))  # csrc/render_variants.h: the `Composite, Actors` rows
LG, ALG = 11, 9  # table sizes: seconds per test
# segment lengths of the ragged test: empty rays, one sample, around one and two tiles, more than one wave's 64 samples
RAGGED = [0, 1, 15, 16, 17, 33, 70, 0, 5, 64, 130, 2, 32, 0, 48, 16]


# ---- scenes ------------------------------------------------------------------------------------------------------------
def street_trajectories(A=20):
    """A parked cars in a row along +x, 5 m apart (the scene of tests/test_gpu_actors.py)"""
    ts, out = torch.tensor([0.0, 1.0]), []
    for a in range(A):
        p = torch.eye(4).repeat(2, 1, 1)
        p[:, :3, 3] = torch.tensor([6.0 + 5.0 * a, 0.3 * (a % 3 - 1), 0.4])
        out.append({"timestamps": ts.clone(), "poses": p, "dims": torch.tensor([2.0, 4.6, 1.6]),
                    "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})
    return out


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict: trajs, o [R,3], d [R,3], area [R], times [R], box0 (level-0 box of a 3-level grid; its level-2 box holds the
    actors), step.  "golden": the rays and times of tests/golden/field_actors.npz with builders.trajectories() -- an overlap,
    an actor present only early.  "street": the 20-actor row, R = 301, every third ray passes nothing."""
    if name == "golden":
        g = load_golden("field_actors")
        return dict(trajs=trajectories(), o=g["o"], d=g["d"], area=g["area"], times=g["times"],
                    box0=np.array([4.0, -4.0, -1.5, 12.0, 4.0, 2.5], f32), step=0.25)
    R = 301
    o = (synth.normal((R, 3), 3) * np.array([0.5, 0.3, 0.1], f32)).astype(f32)
    tgt = np.stack([np.full(R, 110.0), synth.uniform((R,), -0.6, 0.6, 4), synth.uniform((R,), 0.2, 0.6, 5)], -1)
    tgt[::3] = np.stack([synth.uniform((R,), -50, 50, 7), np.full(R, 90.0), synth.uniform((R,), 5, 40, 8)], -1)[::3]  # away
    d = (tgt - o).astype(f32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return dict(trajs=street_trajectories(), o=o, d=d, area=np.full((R,), 2.43e-6, f32),
                times=synth.uniform((R,), 0.0, 1.0, 6), box0=np.array([41.0, -1.5, -0.5, 69.0, 1.5, 1.5], f32), step=0.5)


def level_boxes(box0, levels):
    """[levels, 6]: the three nested boxes of a 3-level grid on box0, or (levels == 1) its outermost box alone"""
    b = np.asarray(OU.level_aabbs(box0, 3), f32)
    return b if levels == 3 else b[2:3]


def random_binaries(levels, res, seed, density=0.3):
    return np.random.default_rng(seed).random((levels, res, res, res)) < density


# ---- fields ------------------------------------------------------------------------------------------------------------
def shape_params(L, F, H, half=False):
    """SDF field of an actor shape with O(1) features; fp16 storage: the oracle sees the rounded table"""
    p = field_params(True, L, F, LG, H, 32, 2048, scale=2.0, seed=70 + L + F)
    p.geo_b[0] = synth.linear(H, 32, 200)[1]
    p.beta = 3.0  # alphas away from saturation: the compositing is exercised
    if half:
        p.grid.table = p.grid.table.astype(np.float16).astype(f32)
    return p


def actor_tables(n, L, F, half=False):
    La = min(4, L)
    tabs = [synth.hash_table(La * 2**ALG, F, seed=900 + i, scale=0.7) for i in range(n)]
    return [t.astype(np.float16).astype(f32) for t in tabs] if half else tabs


def make_actor_field(name, L=8, F=4, H=32, half=False):
    """-> (NeuRADField on the GPU in eval mode, the oracle's FieldParams, the oracle's ActorParams) of scene `name`"""
    from gpu_util import cuda, host, load_field_weights
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    actors = DynamicActors(DynamicActorsConfig(), trajectories=scene(name)["trajs"])
    cfg = NeuRADFieldConfig(geo_hidden_dim=H, nff_hidden_dim=H)
    st, ac = cfg.grid.static, cfg.grid.actor
    st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, 32, 2048, LG
    ac.num_levels, ac.hashgrid_dim, ac.base_res, ac.max_res, ac.log2_hashmap_size = min(4, L), F, 64, 1024, ALG
    p = shape_params(L, F, H, half)
    fld = load_field_weights(NeuRADField(cfg, actors=actors, static_scale=100.0).cuda().eval(), p, half)
    tabs = actor_tables(len(fld.hashgrid.actor_grids), L, F, half)
    with torch.no_grad():
        fld.sdf_to_density.beta.fill_(p.beta)
        for gr, t in zip(fld.hashgrid.actor_grids, tabs):
            if half:
                gr.hash_table.data = cuda(t).half()
            else:
                gr.hash_table.copy_(cuda(t))
    ap = O.ActorParams(host(actors.unique_timestamps), host(actors.actor_positions), host(actors.actor_rotations_6d),
                       host(actors.actor_present_at_time), host(actors.actor_sizes), host(actors.actor_padding),
                       [O.GridParams(t, min(4, L), 64, 1024, ALG) for t in tabs], actor_scale=10.0)
    return fld, p, ap


def oracle_actor_params(name):
    """the oracle's view of scene `name`'s trajectories alone (no GPU): boxes, no grids"""
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    a = DynamicActors(DynamicActorsConfig(), trajectories=scene(name)["trajs"])
    n = lambda t: t.detach().numpy()  # noqa: E731
    return O.ActorParams(n(a.unique_timestamps), n(a.actor_positions), n(a.actor_rotations_6d), n(a.actor_present_at_time),
                         n(a.actor_sizes), n(a.actor_padding), [], actor_scale=10.0)


# ---- the march rule, restated ------------------------------------------------------------------------------------------
def in_box(ap, o, d, times, ray, ts, te, edit=None):
    """[M] bool: is the field's sample position of (ray, ts, te) strictly inside the box of an actor present at the ray's
    time?  fp32, the kernel's order of operations: mean = o + d (t0 + (t1 - t0) / 2), |w2b mean| < bounds per axis."""
    b2w, valid = O.actor_boxes2world(ap, times, edit)
    w2b = O.pose_inverse(b2w)  # [R,A,3,4]
    t0, t1 = np.asarray(ts, f32), np.asarray(te, f32)
    t = (t0 + (t1 - t0) / f32(2)).astype(f32)
    mean = (o[ray] + d[ray] * t[:, None]).astype(f32)  # [M,3]
    pos = np.einsum("makc,mc->mak", w2b[ray][..., :3], mean).astype(f32) + w2b[ray][..., 3]
    return (np.all(np.abs(pos) < ap.bounds[None], axis=-1) & valid[ray]).any(-1)


def march_boxes(aabbs, binaries, o, d, step, box_fn=None, **kw):
    """The box-aware march over a [L,res,res,res] grid (L = 1: occgrid_oracle's single-grid march decides the cells):
    -> (ray_indices, t_starts, t_ends).  box_fn(ray, ts, te) -> [M] bool, None: no candidate boxes at all."""
    aabbs, binaries = np.asarray(aabbs, f32).reshape(-1, 6), np.asarray(binaries).astype(bool)
    if binaries.shape[0] == 1:
        ri, ts, te = OO.occgrid_march(aabbs[0], np.ones_like(binaries[0]), o, d, step, **kw)
        pr, pts, _ = OO.occgrid_march(aabbs[0], binaries[0], o, d, step, **kw)
        keep = np.isin(sample_keys(ri, ts), sample_keys(pr, pts))
    else:
        c = OU.march_levels(aabbs, binaries, o, d, step, **kw)
        ri, ts, te, keep = c["ray"], c["t_start"], c["t_end"], c["keep"]
    if box_fn is not None and ri.shape[0]:
        keep = keep | box_fn(ri, ts, te)
    return ri[keep], ts[keep], te[keep]


def sample_keys(ray, ts):
    """one int64 per (ray, t_start): equal exactly when both are bitwise equal"""
    return (np.asarray(ray, np.int64) << 32) | np.asarray(ts, f32).view(np.uint32).astype(np.int64)


def march_classes(cell, box):
    """-> counts of (cell only, box only, both, neither)"""
    return int((cell & ~box).sum()), int((~cell & box).sum()), int((cell & box).sum()), int((~cell & ~box).sum())


# ---- packed samples and the references of the fused render -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_rays(name, n_rays, seed, t_far=108.0, counts=None):
    """-> o, d, area, times, t_starts [M], t_ends [M], seg [R+1]: the first n_rays rays of scene `name` with RAGGED's segment
    lengths in turn (or `counts`), sorted contiguous intervals inside 0.1 .. t_far"""
    s = scene(name)
    counts = np.asarray([RAGGED[r % len(RAGGED)] for r in range(n_rays)] if counts is None else counts, np.int64)
    rng = np.random.default_rng(seed)
    ts, te = [], []
    for n in counts:
        edges = np.sort(rng.uniform(0.1, t_far, int(n) + 1)).astype(f32)
        ts.append(edges[:-1]), te.append(edges[1:])
    cat = lambda parts: np.concatenate(parts).astype(f32) if parts else np.zeros((0,), f32)  # noqa: E731
    return (s["o"][:n_rays], s["d"][:n_rays], s["area"][:n_rays], s["times"][:n_rays], cat(ts), cat(te),
            PR.segments_from_counts(counts))


def oracle_route(p, ap, rays, edit=None):
    """The numpy oracle per sample, composited in float64 by tests/packed_restatement.py.  The oracle culls actors by the
    ray's line through its first and last sample, so every segment is laid into a dense row between two far-apart dummy
    samples and the live entries are picked out again."""
    o, d, area, times, ts, te, seg = rays
    counts = np.diff(seg)
    R, S = len(counts), int(counts.max()) + 2
    st, en = np.full((R, S), 0.01, f32), np.full((R, S), 0.02, f32)
    st[:, -1], en[:, -1] = 150.0, 151.0
    for r in range(R):
        st[r, 1:1 + counts[r]], en[r, 1:1 + counts[r]] = ts[seg[r]:seg[r + 1]], te[seg[r]:seg[r + 1]]
    f = O.field_fwd_actors(p, ap, o, d, area, st, en, times, edit=edit)
    live = (np.arange(S)[None] >= 1) & (np.arange(S)[None] < 1 + counts[:, None])
    feat, depth, acc, w = PR.composite(PR.f64(ts), PR.f64(te), PR.f64(f["alpha"][live]), PR.f64(f["feature"][live]), seg, False)
    return feat.numpy(), depth.numpy(), acc.numpy(), w.numpy()


def bundle_of(rays):
    from gpu_util import cuda
    from neurad_studio_amd.cameras.rays import RayBundle

    o, d, area, times = rays[:4]
    return RayBundle(origins=cuda(o), directions=cuda(d), pixel_area=cuda(area)[:, None], times=cuda(times)[:, None])


def operator_route(fld, rays):
    """the route packed samples of an actor scene took before the fused kernel: per-sample gathers -> field(rs) [M,1] ->
    renderers.render_packed"""
    from gpu_util import cuda
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.model_components.renderers import render_packed

    rb, R = bundle_of(rays), rays[0].shape[0]
    ri = cuda(PR.ray_indices_from_segments(rays[6]))
    with torch.no_grad():
        rs = VolumetricSampler._gather(rb, rb.origins, rb.directions, ri, cuda(rays[4]), cuda(rays[5]))
        out = fld(rs)
        got = render_packed(out[FieldHeadNames.FEATURE], rs, ri, R, alpha=out[FieldHeadNames.ALPHA])
    return got["features"], got["depth"], got["accumulation"], got["weights"][:, 0]


def fused_route(fld, rays, **kw):
    from gpu_util import cuda

    o, d, area, times, ts, te, seg = (cuda(a) for a in rays)
    with torch.no_grad():
        return fld.render_packed(o, d, area, ts, te, segments=seg, times=times, return_weights=True, **kw)


def close(got, want, bound, what):
    """the comparison of tests/test_gpu_render_packed.py: rel-L2 per output (depth: or 1e-5 absolute)"""
    for name, g, w in zip(("features", "depth", "accumulation", "weights"), got, want):
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g
        w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w
        err = rel_l2(g.reshape(-1), w.reshape(-1))
        print(f"{what} {name}: rel-L2 {err:.3e} (bound {bound:g})")
        assert err < bound or (name == "depth" and np.abs(g.reshape(-1) - w.reshape(-1)).max() < 1e-5), (what, name, err)


def sample_hits(ops, spec, cand, o, d, area, ri, ts, te):
    """[M] int32: the actor whose box contains each packed sample (-1: none), by the field's own kernel -- ops.actor_encode
    on M rays of one sample with the sample's ray's candidate list"""
    M = ri.shape[0]
    if M == 0:
        return torch.zeros((0,), dtype=torch.int32, device=o.device)
    per_sample = (cand[0][ri].contiguous(), cand[1][ri].contiguous(), cand[2][ri].contiguous(), None)
    feats = torch.zeros((M, 32), device=o.device)
    return ops.actor_encode(spec, per_sample, o[ri], d[ri], area.reshape(-1)[ri], ts[:, None], te[:, None], feats)[1]
