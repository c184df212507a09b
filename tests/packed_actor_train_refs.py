"""What the tests of the fused training node for packed samples with dynamic actors share
(tests/test_gpu_packed_actor_train.py): training-mode fields on the scenes of tests/packed_actor_refs.py, their static twins,
rays without candidates, uniform segments (packed samples that are also a dense [R,S] batch), the operator route with
autograd, the route runner and the comparison at the bounds of tests/test_gpu_render_train_packed.py (compare_routes: 2e-5
outputs, 2e-4 parameter gradients, 1e-3 beta).  No kernel code is shared."""
import functools

import numpy as np
import torch

import neurad_oracle as O
import packed_actor_refs as PA
import packed_restatement as PR
import synth
from builders import field_params
from conftest import rel_l2

f32 = np.float32
OUT_NAMES = ("features", "depth", "accumulation", "weights")


# ---- rays --------------------------------------------------------------------------------------------------------------
def uniform_rays(name, n_rays, S, seed=7, t_far=108.0):
    """ragged_rays with S samples on every ray: the packed arrays are the rows of a dense [R,S] batch"""
    return PA.ragged_rays(name, n_rays, seed, t_far, counts=(S,) * n_rays)


@functools.lru_cache(maxsize=None)
def subset_rays(name, first, step, n_rays, seed, counts=None):
    """ragged_rays over the rays first, first + step, ... of scene `name` (RAGGED's lengths in turn, or `counts`)"""
    s = PA.scene(name)
    idx = first + step * np.arange(n_rays)
    counts = np.asarray([PA.RAGGED[r % len(PA.RAGGED)] for r in range(n_rays)] if counts is None else counts, np.int64)
    rng = np.random.default_rng(seed)
    ts, te = [], []
    for n in counts:
        edges = np.sort(rng.uniform(0.1, 108.0, int(n) + 1)).astype(f32)
        ts.append(edges[:-1]), te.append(edges[1:])
    cat = lambda parts: np.concatenate(parts).astype(f32) if parts else np.zeros((0,), f32)  # noqa: E731
    return (s["o"][idx], s["d"][idx], s["area"][idx], s["times"][idx], cat(ts), cat(te), PR.segments_from_counts(counts))


def on_device(rays):
    """-> o, d, area, times, ts, te, seg int64, ray_indices int64 on the GPU"""
    from gpu_util import cuda

    return (*(cuda(a) for a in rays), cuda(PR.ray_indices_from_segments(rays[6])))


def sample_stats(name, rays):
    """From the data, on the CPU (the oracle's box test, packed_actor_refs.in_box's arithmetic per actor): -> dict with the
    number of samples M, in-box samples, (sample, actor) pairs, samples in two or more boxes, rays with hits, actors hit"""
    o, d, area, times, ts, te, seg = rays
    ap = PA.oracle_actor_params(name)
    ri = PR.ray_indices_from_segments(seg)
    b2w, valid = O.actor_boxes2world(ap, times, None)
    w2b = O.pose_inverse(b2w)
    t = (ts + (te - ts) / f32(2)).astype(f32)
    mean = (o[ri] + d[ri] * t[:, None]).astype(f32)
    pos = np.einsum("makc,mc->mak", w2b[ri][..., :3], mean).astype(f32) + w2b[ri][..., 3]
    inside = np.all(np.abs(pos) < ap.bounds[None], axis=-1) & valid[ri]  # [M, A]
    per = inside.sum(-1)
    return dict(M=int(ts.shape[0]), in_box=int((per > 0).sum()), pairs=int(per.sum()), overlap=int((per > 1).sum()),
                rays_hit=int(np.unique(ri[per > 0]).shape[0]), actors_hit=int(inside.any(0).sum()),
                n_actors=int(inside.shape[1]))


# ---- fields ------------------------------------------------------------------------------------------------------------
def _shape_params(L, F, H, half, lg):
    if lg == PA.LG:
        return PA.shape_params(L, F, H, half)
    p = field_params(True, L, F, lg, H, 32, 2048, scale=2.0, seed=70 + L + F)  # shape_params on a larger table
    p.geo_b[0] = synth.linear(H, 32, 200)[1]
    p.beta = 3.0
    if half:
        p.grid.table = p.grid.table.astype(np.float16).astype(f32)
    return p


def _density_head(fld):
    """the field with the density head (use_sdf = False): the geometry MLP's first output scaled to O(1) logits"""
    fld.config.use_sdf = False
    with torch.no_grad():
        fld.mlp_geo.layers[1].weight[0].mul_(0.25)
        fld.mlp_geo.layers[1].bias[0].mul_(0.25)
    return fld


def make_train_field(name, L=8, F=4, H=32, half=False, use_sdf=True, flip_prob=0.0, lg=PA.LG):
    """-> (NeuRADField with scene `name`'s actors in TRAINING mode, the oracle's FieldParams and ActorParams).  Every call
    builds the same weights (packed_actor_refs.make_actor_field; lg: another static table size)."""
    if lg == PA.LG:
        fld, p, ap = PA.make_actor_field(name, L, F, H, half)
    else:
        from gpu_util import cuda, load_field_weights
        from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
        from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

        actors = DynamicActors(DynamicActorsConfig(), trajectories=PA.scene(name)["trajs"])
        cfg = NeuRADFieldConfig(geo_hidden_dim=H, nff_hidden_dim=H)
        st, ac = cfg.grid.static, cfg.grid.actor
        st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, 32, 2048, lg
        ac.num_levels, ac.hashgrid_dim, ac.base_res, ac.max_res, ac.log2_hashmap_size = min(4, L), F, 64, 1024, PA.ALG
        p, ap = _shape_params(L, F, H, half, lg), None
        fld = load_field_weights(NeuRADField(cfg, actors=actors, static_scale=100.0).cuda(), p, half)
        with torch.no_grad():
            fld.sdf_to_density.beta.fill_(p.beta)
            for gr, t in zip(fld.hashgrid.actor_grids, PA.actor_tables(len(fld.hashgrid.actor_grids), L, F, half)):
                if half:
                    gr.hash_table.data = cuda(t).half()
                else:
                    gr.hash_table.copy_(cuda(t))
    fld.train()
    fld.hashgrid.config.actor.flip_prob = flip_prob
    return (fld if use_sdf else _density_head(fld)), p, ap


def make_static_twin(L=8, F=4, H=32, half=False, use_sdf=True):
    """the field of make_train_field built WITHOUT actors, same static table, MLPs and beta, training mode"""
    from gpu_util import load_field_weights
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig

    cfg = NeuRADFieldConfig(geo_hidden_dim=H, nff_hidden_dim=H)
    st = cfg.grid.static
    st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, 32, 2048, PA.LG
    p = PA.shape_params(L, F, H, half)
    fld = load_field_weights(NeuRADField(cfg, actors=None, static_scale=100.0).cuda(), p, half).train()
    with torch.no_grad():
        fld.sdf_to_density.beta.fill_(p.beta)
    return fld if use_sdf else _density_head(fld)


def static_grid(name, res=32):
    """an estimator as a grid trained on the static density has it: random cells, none near the actors (the grid of
    tests/test_gpu_packed_actors.py's sampler tests, restated)"""
    from gpu_util import cuda
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    s = PA.scene(name)
    boxes = PA.level_boxes(s["box0"], 3)
    est = OccGridEstimator(boxes[2].tolist(), resolution=res)
    binaries = PA.random_binaries(1, res, 3)[0]
    lo, hi = boxes[2][:3], boxes[2][3:]
    centres = np.stack(np.meshgrid(*[lo[a] + (np.arange(res) + 0.5) * (hi[a] - lo[a]) / res for a in range(3)], indexing="ij"), -1)
    pos = PA.oracle_actor_params(name).positions.reshape(-1, 3)  # every actor at every stored time
    binaries &= ~(np.linalg.norm(centres[..., None, :] - pos, axis=-1) < 5.0).any(-1)
    est.binaries[0] = cuda(binaries)
    return est


# ---- routes ------------------------------------------------------------------------------------------------------------
def operator_route(fld, dr):
    """the route the node replaces, with autograd: per-sample gathers -> field(rs) [M,1] -> renderers.render_packed.  In
    training mode the x-flip is drawn per gathered "ray", i.e. per SAMPLE."""
    from neurad_studio_amd.cameras.rays import RayBundle
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.model_components.renderers import render_packed

    o, d, area, times, ts, te, seg, ri = dr
    rb = RayBundle(origins=o, directions=d, pixel_area=area[:, None], times=times[:, None])
    rs = VolumetricSampler._gather(rb, o, d, ri, ts, te)
    out = fld(rs)
    kw = {"alpha": out[FH.ALPHA]} if FH.ALPHA in out else {"density": out[FH.DENSITY]}
    got = render_packed(out[FH.FEATURE], rs, ri, o.shape[0], **kw)
    return got["features"], got["depth"], got["accumulation"], got["weights"][:, 0]


def node_route(fld, dr, **kw):
    o, d, area, times, ts, te, seg, ri = dr
    return fld.render_train_packed(o, d, area, ts, te, segments=seg, times=times, **kw)


def cotangents(R, M, seed=81):
    """the pattern of tests/test_gpu_render_train_packed.py"""
    from gpu_util import dev

    return (dev(synth.normal((R, 32), seed)), dev(synth.normal((R, 1), seed + 1)), dev(synth.normal((R, 1), seed + 2)),
            dev(synth.normal((M,), seed + 3)))


def field_grads(fld):
    from packed_train_refs import field_grads as fg

    return fg(fld)


def run_route(fld, dr, route, cot):
    """-> [features, depth, accumulation, weights], {parameter name: gradient}"""
    outs = route(fld, dr)
    sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot)).backward()
    return [t.detach() for t in outs], field_grads(fld)


TABLE = "hashgrid.static_grid.hash_table"


def compare_routes(node, operator, what=""):
    """compare_routes of tests/test_gpu_render_train_packed.py with every figure printed first: outputs at 2e-5, gradients at
    2e-4 rel-L2 (beta: 1e-3), same parameters with a gradient, same dtypes"""
    from gpu_util import host64

    (fo, fg), (oo, og) = node, operator
    failed = []
    for name, a, b in zip(OUT_NAMES, fo, oo):
        err = rel_l2(host64(a).reshape(-1), host64(b).reshape(-1))
        print(f"{what}{name}: node vs operator rel-L2 {err:.3e} (bound 2e-05)")
        if not err < 2e-5:
            failed.append((name, err))
    assert set(fg) == set(og), set(fg) ^ set(og)
    for n in sorted(fg):
        bound = 1e-3 if n == "sdf_to_density.beta" else 2e-4
        a, b = host64(fg[n].float()).reshape(-1), host64(og[n].float()).reshape(-1)
        err = rel_l2(a, b) if np.abs(b).max() > 0 else float(np.abs(a).max())
        print(f"{what}d {n}: node vs operator rel-L2 {err:.3e} (bound {bound:g}; |operator| max {np.abs(b).max():.3e})")
        if not (fg[n].dtype == og[n].dtype and err < bound):
            failed.append((n, err))
    assert not failed, failed
