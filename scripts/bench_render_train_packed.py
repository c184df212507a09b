"""A training step's field part on occupancy-marched (packed) samples, two ways, at a size a user would run: 16 384 rays
with march-like ragged sample counts (mean ~32 per ray, a tenth of the rays empty, a tail past 100), NeuRAD's default field
(8 levels x 4 features, width 32, SDF head with the learnable beta), an fp32 table of 2^19 entries per level.  Forward +
backward (gradients of the table, the ten MLP tensors and beta), timed with device events after a warm-up, alternating in
one process:
  (a) the fused node of VolumetricSampler.render_train: NeuRADField.render_train_packed on the bundle's per-ray tensors
      (autograd.NffRenderTrainFn on autograd.PackedSamples);
  (b) the operator route: per-sample gathers of origins / directions / pixel area, the field on [M,1] (FieldTrainFn, every
      sample a ray of one sample), the torch head, renderers.render_packed (PackedCompositeFn).
Appends ONE JSON line (M, the segment-length histogram, device clocks under load, medians, the ratio (b)/(a), and the rel-L2
of (a) against (b) on outputs and gradients) to profiles/bench_render_train_packed.jsonl.  Fails without a GPU.
--ray-grads: the same two routes at the same size with origins and directions that REQUIRE GRAD (a camera optimizer moved
them), their two gradients added to what each step computes: (a) is the node with ray_gradients=True (its ray gradients from
nrhip_encode_bwd_rays_packed), (b) the fallback VolumetricSampler.render_train takes by default for such rays (the gathers'
index_add_ backward folds the per-sample rows to rays).  The line's "bench" is then "render_train_packed_ray_grads".
--actors: the street scene of scripts/bench_render_packed.py --actors (65 536 rays, 24 moving actors, the box-aware march's
packed samples, NeuRAD's default field with 4 x 4 actor grids) in training mode, flip_prob = 0 (the two routes draw the flip
differently: per ray against per sample; a non-zero flip is not measured).  The march and the per-ray candidate lists are
outside the timed region; timed, alternating, forward + backward (static table, MLPs, beta, the 24 actor tables, the
trajectories):
  (a) NeuRADField.render_train_packed(..., times=..., actor_cand=...): autograd.NffRenderTrainFn with row overrides;
  (b) the operator route on the same samples: gathers, the field with actors on [M,1], the torch head, renderers.render_packed
      (what VolumetricSampler.render_train(..., actor_boxes=True) does by default; it computes its own per-sample lists).
The line's "bench" is "render_train_packed_actors".  No ratio is promised.
--actors --ray-grads: the same scene and the same two routes with origins and directions that REQUIRE GRAD, their two
gradients added to what each step computes: (a) is the node with actor_ray_gradients=True (the static share from
nrhip_encode_bwd_rays_packed, the in-box samples' from nrhip_actor_pair_positions_bwd_rays_packed), (b) the operator route
with the same moving rays (what VolumetricSampler.render_train takes for them by default).  The line's "bench" is
"render_train_packed_actors_ray_grads".  No ratio is promised.
--actors --pair-kernels: no timing of its own -- the pair backward of the scene's pairs, 20 launches each, for ONE kernel
trace (rocprofv3 --kernel-trace --stats -- python scripts/bench_render_train_packed.py --actors --pair-kernels): the new
kernel actor_pair_positions_bwd_rays_packed_kernel; actor_pair_positions_bwd_kernel<PackedRaysDev>, the trajectory gradients
that stay beside it; and actor_pair_positions_bwd_kernel<RaysDev> with ray gradients on the same pairs laid out as the
operator route lays them out ([M,1] rays), the dense atomic kernel that does both.  Prints the pair count; writes no line.
    python scripts/bench_render_train_packed.py [--ray-grads] [--actors [--pair-kernels]] [--reps 100] [--warmup 10] [--out profiles/bench_render_train_packed.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neurad_studio_amd.cameras.rays import RayBundle  # noqa: E402
from neurad_studio_amd.field_components.field_heads import FieldHeadNames  # noqa: E402
from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig  # noqa: E402
from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler  # noqa: E402
from neurad_studio_amd.model_components.renderers import render_packed  # noqa: E402

R, LOG2_T, STEP = 16384, 19, 0.05
L, F, H, BASE, MAX_RES = 8, 4, 32, 32, 8192


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def median(v):
    return sorted(v)[len(v) // 2]


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def make_field(gen):
    cfg = NeuRADFieldConfig(geo_hidden_dim=H, nff_hidden_dim=H, sdf_beta=3.0)
    st = cfg.grid.static
    st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, BASE, MAX_RES, LOG2_T
    torch.manual_seed(1)
    f = NeuRADField(cfg, actors=None, static_scale=4.0).cuda().train()
    with torch.no_grad():  # a table with structure (the initialisation's 1e-4 entries give one flat alpha)
        t = f.hashgrid.static_grid.hash_table
        t.copy_(((torch.rand(t.shape, generator=gen) * 2 - 1) * 0.5).to(t.device))
    return f


def ragged_samples(rng):
    """march-like counts: a tenth of the rays miss everything, the rest cross gamma-distributed lengths of occupied space"""
    counts = np.minimum(rng.gamma(2.0, 18.0, R), 200.0).astype(np.int64)
    counts[rng.random(R) < 0.1] = 0
    seg = np.zeros(R + 1, np.int64)
    np.cumsum(counts, out=seg[1:])
    ri = np.repeat(np.arange(R, dtype=np.int64), counts)
    k = np.arange(seg[-1], dtype=np.int64) - seg[ri]
    near = rng.uniform(0.05, 1.0, R).astype(np.float32)
    ts = near[ri] + STEP * k.astype(np.float32)
    return counts, ri, ts.astype(np.float32), (ts + np.float32(STEP)).astype(np.float32)


def main_actors(args):
    import bench_render_packed as BP  # (scripts/ is sys.path[0]: the scene is that script's)
    from bench import device_state

    sc = BP.actor_scene()
    fld, o, d, area, times, cand, ri, ts, te, seg = (sc[k] for k in ("fld", "o", "d", "area", "times", "cand", "ri", "ts", "te", "seg"))
    rays, M = o.shape[0], int(ri.shape[0])
    counts = (seg[1:] - seg[:-1]).cpu().numpy()
    fld.train()
    fld.hashgrid.config.actor.flip_prob = 0.0
    assert fld.fused_packed_actors_train_supported()
    if args.pair_kernels:
        return pair_kernels(fld, o, d, area, times, cand, ri, ts, te, seg)
    node_kw = {}
    if args.ray_grads:
        o, d = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        node_kw = {"actor_ray_gradients": True}
    rb = RayBundle(origins=o, directions=d, pixel_area=area, times=times[:, None])
    cot = [torch.randn(s, generator=sc["gen"]).cuda() for s in ((rays, 32), (rays, 1), (rays, 1), (M,))]
    named = [(n, p) for n, p in fld.named_parameters() if p.requires_grad]
    names, params = [n for n, _ in named], [p for _, p in named]
    if args.ray_grads:
        names, params = names + ["origins", "directions"], params + [o, d]

    def loss_of(outs):
        return sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot))

    def route_a():
        outs = fld.render_train_packed(o, d, area, ts, te, ray_indices=ri, num_rays=rays, times=times, actor_cand=cand,
                                       **node_kw)
        return outs, torch.autograd.grad(loss_of(outs), params, allow_unused=True)

    def route_b():
        rs = VolumetricSampler._gather(rb, o, d, ri, ts, te)
        out = fld(rs)
        res = render_packed(out[FieldHeadNames.FEATURE], rs, ri, rays, alpha=out[FieldHeadNames.ALPHA])
        outs = (res["features"], res["depth"], res["accumulation"], res["weights"][:, 0])
        return outs, torch.autograd.grad(loss_of(outs), params, allow_unused=True)

    (oa, ga), (ob, gb) = route_a(), route_b()
    agree = {k: rel_l2(x, y) for k, x, y in zip(("features", "depth", "accumulation", "weights"), oa, ob)}
    tabs = [rel_l2(x, y) for n, x, y in zip(names, ga, gb) if x is not None and y is not None and ".actor_grids." in n]
    agree.update({f"d {n}": rel_l2(x, y) for n, x, y in zip(names, ga, gb)
                  if x is not None and y is not None and ".actor_grids." not in n})
    agree["d actor tables (max of %d)" % len(tabs)] = max(tabs)
    del oa, ga, ob, gb
    keys = ("a_fused_node_actors", "b_operator_route")
    lap = {k: [] for k in keys}
    clocks = device_state(0)
    for rep in range(args.warmup + args.reps):
        for key, fn in zip(keys, (route_a, route_b)):  # alternating
            t = timed(fn)
            if rep >= args.warmup:
                lap[key].append(t)
    med = {k: median(v) for k, v in lap.items()}
    acfg = sc["cfg"].grid.actor
    line = {
        "bench": "render_train_packed_actors" + ("_ray_grads" if args.ray_grads else ""),
        "field": "neurad_default_8x4_h32", "levels": L, "features_per_level": F,
        "hidden": H, "head": "sdf", "log2_table": BP.LOG2_T, "table_dtype": "fp32", "actors": int(sc["actors"].n_actors),
        "actor_grid": [acfg.num_levels, acfg.hashgrid_dim, acfg.log2_hashmap_size], "flip_prob": 0.0,
        "rays": rays, "grid": BP.RES, "step": BP.STEP, "M": M, "M_plain_march": sc["plain_m"],
        "rays_with_candidates": float((cand[0] > 0).float().mean()),
        "segments": {"min": int(counts.min()), "median": float(np.median(counts)), "p99": float(np.percentile(counts, 99)),
                     "max": int(counts.max()), "empty_share": float((counts == 0).mean())},
        "device": torch.cuda.get_device_name(0), "clocks_under_load": clocks, "reps": args.reps, "warmup": args.warmup,
        "median_us": med, "min_us": {k: min(v) for k, v in lap.items()}, "max_us": {k: max(v) for k, v in lap.items()},
        "ratio_b_over_a": med[keys[1]] / med[keys[0]],
        "note": "forward + backward; march and per-ray candidate lists outside the timed region; (b) computes its own "
                "per-sample lists",
        "a_vs_b_rel_l2": agree,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


def pair_kernels(fld, o, d, area, times, cand, ri, ts, te, seg, launches=20):
    """the three pair-backward kernels on the scene's pairs, for a kernel trace (see the module docstring)"""
    from neurad_studio_amd import ops

    hg = fld.hashgrid
    spec = hg.actor_spec()
    a = area.reshape(-1)
    with torch.no_grad():
        hits = ops.actor_find_packed(spec, cand, o, d, a, ts, te, ri)[0]
        si, ai = ops.actor_pairs(hits)
        P = int(si.shape[0])
        gen = torch.Generator().manual_seed(3)
        gx, gc = torch.randn((P, 3), generator=gen).cuda(), torch.randn((P,), generator=gen).cuda()
        og, dg, ag, tg = o[ri], d[ri], a[ri], times[ri]  # the operator route's layout: every sample a ray of one sample
        for _ in range(launches):
            ops.actor_pair_positions_packed_bwd_rays(spec, o, d, a, ts, te, seg, times, si, ai, None, gx, gc)
            ops.actor_pair_positions_packed_bwd(spec, o, d, a, ts, te, ri, times, si, ai, None, gx, gc)
            ops.actor_pair_positions_bwd(spec, og, dg, ag, ts[:, None], te[:, None], tg, si, ai, None, gx, gc, ray_grads=True)
        torch.cuda.synchronize()
    print(json.dumps({"pair_kernels": {"pairs": P, "rays": int(o.shape[0]), "M": int(ri.shape[0]), "launches": launches}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ray-grads", action="store_true", help="rays that require grad: the opt-in node against the fallback")
    ap.add_argument("--actors", action="store_true", help="the fused node with dynamic actors against the operator route")
    ap.add_argument("--pair-kernels", action="store_true", help="with --actors: launch the pair-backward kernels for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_render_train_packed.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_train_packed: no GPU")
    if args.pair_kernels and not args.actors:
        raise SystemExit("bench_render_train_packed: --pair-kernels needs --actors")
    if args.actors:
        return main_actors(args)
    from bench import device_state

    gen = torch.Generator().manual_seed(0)
    counts, ri, ts, te = ragged_samples(np.random.default_rng(0))
    M = int(ri.shape[0])
    o = ((torch.rand((R, 3), generator=gen) * 2 - 1) * 3.5).cuda()
    d = torch.nn.functional.normalize(torch.randn((R, 3), generator=gen), dim=-1).cuda()
    if args.ray_grads:
        o.requires_grad_(True), d.requires_grad_(True)
    area = torch.full((R, 1), 2.4e-6, device="cuda")
    ri, ts, te = torch.from_numpy(ri).cuda(), torch.from_numpy(ts).cuda(), torch.from_numpy(te).cuda()
    rb = RayBundle(origins=o, directions=d, pixel_area=area)
    cot = [torch.randn(s, generator=gen).cuda() for s in ((R, 32), (R, 1), (R, 1), (M,))]
    fld = make_field(gen)
    assert fld.fused_packed_train_supported()
    params = [p for p in fld.parameters() if p.requires_grad] + ([o, d] if args.ray_grads else [])
    names = [n for n, p in fld.named_parameters() if p.requires_grad] + (["origins", "directions"] if args.ray_grads else [])

    def loss_of(outs):
        return sum((t.reshape(c.shape) * c).sum() for t, c in zip(outs, cot))

    def route_a():
        outs = fld.render_train_packed(o, d, area, ts, te, ray_indices=ri, num_rays=R, ray_gradients=args.ray_grads)
        return outs, torch.autograd.grad(loss_of(outs), params, allow_unused=True)

    def route_b():
        fld.fused_training = True  # (FieldTrainFn on the [M,1] rays: the parent's training path for packed samples)
        rs = VolumetricSampler._gather(rb, o, d, ri, ts, te)
        out = fld(rs)
        res = render_packed(out[FieldHeadNames.FEATURE], rs, ri, R, alpha=out[FieldHeadNames.ALPHA])
        outs = (res["features"], res["depth"], res["accumulation"], res["weights"][:, 0])
        return outs, torch.autograd.grad(loss_of(outs), params, allow_unused=True)

    (oa, ga), (ob, gb) = route_a(), route_b()
    agree = {k: rel_l2(x, y) for k, x, y in zip(("features", "depth", "accumulation", "weights"), oa, ob)}
    agree.update({f"d {n}": rel_l2(x, y) for n, x, y in zip(names, ga, gb) if x is not None})
    times = {"a_fused_node": [], "b_operator_route": []}
    clocks = device_state(0)  # (sampled under a load of its own)
    for rep in range(args.warmup + args.reps):
        for key, fn in (("a_fused_node", route_a), ("b_operator_route", route_b)):  # alternating
            t = timed(fn)
            if rep >= args.warmup:
                times[key].append(t)
    med = {k: median(v) for k, v in times.items()}
    line = {
        "bench": "render_train_packed_ray_grads" if args.ray_grads else "render_train_packed",
        "field": "neurad_default_8x4_h32", "levels": L, "features_per_level": F, "hidden": H,
        "head": "sdf", "log2_table": LOG2_T, "table_dtype": "fp32", "rays": R, "M": M,
        "segments": {"min": int(counts.min()), "mean": float(counts.mean()), "median": float(np.median(counts)),
                     "p99": float(np.percentile(counts, 99)), "max": int(counts.max()),
                     "empty_share": float((counts == 0).mean())},
        "device": torch.cuda.get_device_name(0), "clocks_under_load": clocks, "reps": args.reps, "warmup": args.warmup,
        "median_us": med, "min_us": {k: min(v) for k, v in times.items()}, "max_us": {k: max(v) for k, v in times.items()},
        "ratio_b_over_a": med["b_operator_route"] / med["a_fused_node"],
        "a_vs_b_rel_l2": agree,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
