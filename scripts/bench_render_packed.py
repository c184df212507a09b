"""An eval render of occupancy-marched samples, two ways, at a size a user would run: 65 536 rays marched through a 128^3
occupancy grid at ~30 % occupancy (O(100) samples per hitting ray), NeuRAD's default field (8 levels x 4 features, width 32)
and BASELINE config[1]'s (16 x 2, width 64), fp32 tables of 2^19 entries per level.  The march is outside the timed region.
Timed with device events after a warm-up, alternating in one process:
  (a) the fused packed route of VolumetricSampler.render: NeuRADField.render_packed on the bundle's per-ray tensors
      (segments from ray_indices + nrhip_render_fwd_packed);
  (b) the route the packed samples took before: per-sample gathers of origins / directions / pixel area, the field on
      [M,1] (every sample a ray of one sample), renderers.render_packed (segments + nrhip_packed_composite_fwd).
Appends ONE JSON line per field (M, the segment-length histogram, device clocks, medians, the ratio (b)/(a), (a)'s
algorithmic bytes M (L 8 F sizeof + 8) + R (40 + 136) over its time as a share of the 8 TB/s HBM peak -- a WHOLE-CALL
figure -- and the rel-L2 of (a) against (b) on a 1 024-ray slice) to profiles/bench_render_packed.jsonl.  Fails without a GPU.
--actors: the same size with a street of 24 moving actors (two rows of 12 boxes through the grid, their cells cleared as a grid
built from static densities has them) and NeuRAD's default field with 4 x 4 actor grids.  The box-aware march and the per-ray
candidate lists are outside the timed region; timed, alternating:
  (a) NeuRADField.render_packed(..., actor_cand=...): segments + nrhip_render_fwd_packed_actors;
  (b) the operator route on the same samples: gathers, the field with actors on [M,1], renderers.render_packed.
Appends ONE line ("bench": "render_packed_actors").  No ratio is promised: nobody had measured either route with actors.
    python scripts/bench_render_packed.py [--actors] [--reps 20] [--warmup 5] [--out profiles/bench_render_packed.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neurad_studio_amd import ops  # noqa: E402
from neurad_studio_amd.cameras.rays import RayBundle  # noqa: E402
from neurad_studio_amd.field_components.field_heads import FieldHeadNames  # noqa: E402
from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig  # noqa: E402
from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler  # noqa: E402
from neurad_studio_amd.model_components.renderers import render_packed  # noqa: E402

HBM_PEAK = 8e12  # bytes/s
R, RES, STEP, LOG2_T, TOL = 65536, 128, 0.0125, 19, 1e-5
FIELDS = {"neurad_default_8x4_h32": (8, 4, 32, 32, 8192), "config1_16x2_h64": (16, 2, 64, 16, 1024)}  # L, F, H, base, max res


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


def make_field(L, F, H, base, max_res, gen):
    cfg = NeuRADFieldConfig(geo_hidden_dim=H, nff_hidden_dim=H)
    st = cfg.grid.static
    st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, base, max_res, LOG2_T
    torch.manual_seed(1)
    f = NeuRADField(cfg, actors=None, static_scale=4.0).cuda().eval()
    with torch.no_grad():  # a table with structure (the initialisation's 1e-4 entries give one flat alpha)
        t = f.hashgrid.static_grid.hash_table
        t.copy_(((torch.rand(t.shape, generator=gen) * 2 - 1) * 0.5).to(t.device))
    return f


def street(n_per_row=12):
    """two rows of boxes along x through the grid, moving 0.2 m between the two timestamps"""
    out = []
    for a in range(2 * n_per_row):
        row, k = divmod(a, n_per_row)
        p = torch.eye(4).repeat(2, 1, 1)
        p[:, :3, 3] = torch.tensor([-3.3 + 0.6 * k, -0.9 + 1.8 * row, -0.2 + 0.05 * (a % 3)])
        p[1, 0, 3] += 0.2
        out.append({"timestamps": torch.tensor([0.0, 1.0]), "poses": p, "dims": torch.tensor([0.2, 0.45, 0.16]),
                    "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})
    return out


def actor_scene():
    """The street scene of --actors (scripts/bench_render_train_packed.py --actors trains on the same samples): the field in
    eval mode, its actors, the grid's binaries, the rays, their candidate lists and the box-aware march's packed samples"""
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    gen = torch.Generator().manual_seed(0)
    L, F, H, base, max_res = FIELDS["neurad_default_8x4_h32"]
    cfg = NeuRADFieldConfig(geo_hidden_dim=H, nff_hidden_dim=H)
    st = cfg.grid.static
    st.num_levels, st.hashgrid_dim, st.base_res, st.max_res, st.log2_hashmap_size = L, F, base, max_res, LOG2_T
    actors = DynamicActors(DynamicActorsConfig(actor_bbox_padding=(0.05, 0.05, 0.02)), trajectories=street())
    torch.manual_seed(1)
    fld = NeuRADField(cfg, actors=actors, static_scale=4.0).cuda().eval()
    with torch.no_grad():
        for t in [fld.hashgrid.static_grid.hash_table] + [g.hash_table for g in fld.hashgrid.actor_grids]:
            t.copy_(((torch.rand(t.shape, generator=gen) * 2 - 1) * 0.5).to(t.device))
    assert fld.fused_packed_actors_supported()
    binaries = torch.rand((RES, RES, RES), generator=gen) < 0.3
    centres = (torch.arange(RES) + 0.5) * (8.0 / RES) - 4.0
    cx, cy, cz = torch.meshgrid(centres, centres, centres, indexing="ij")
    cells = torch.stack([cx, cy, cz], -1)
    radius = float(actors.actor_bounds().detach().norm(dim=-1).max()) + 0.3
    for pos in actors.actor_positions.detach().cpu().reshape(-1, 3):  # cleared where an actor ever is
        binaries &= (cells - pos).norm(dim=-1) > radius
    binaries = binaries.cuda()
    o = ((torch.rand((R, 3), generator=gen) * 2 - 1) * 3.5).cuda()
    d = torch.nn.functional.normalize(torch.randn((R, 3), generator=gen), dim=-1).cuda()
    area = torch.full((R, 1), 2.4e-6, device="cuda")
    times = torch.rand((R,), generator=gen).cuda()
    grid = ops.OccGridSpec(torch.tensor([-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]), binaries)
    spec, cand = fld.hashgrid.prepare_actors_line(o, d, 0.0, 1.0, times)
    plain_m = int(ops.occgrid_march(grid, o, d, STEP)[0].shape[0])
    ri, ts, te, seg = ops.occgrid_march(grid, o, d, STEP, actor_boxes=(spec, cand))
    return dict(cfg=cfg, fld=fld, actors=actors, binaries=binaries, o=o, d=d, area=area, times=times, cand=cand,
                plain_m=plain_m, ri=ri, ts=ts, te=te, seg=seg, gen=gen)


def main_actors(args):
    from bench import device_state

    clocks = device_state(0)
    sc = actor_scene()
    L, F, H, _, _ = FIELDS["neurad_default_8x4_h32"]
    cfg, fld, actors, binaries, o, d, area, times, cand = (sc[k] for k in ("cfg", "fld", "actors", "binaries", "o", "d", "area",
                                                                            "times", "cand"))
    plain_m, ri, ts, te, seg = (sc[k] for k in ("plain_m", "ri", "ts", "te", "seg"))
    A = int(actors.n_actors)
    M = int(ri.shape[0])
    counts = (seg[1:] - seg[:-1]).cpu().numpy()
    rb = RayBundle(origins=o, directions=d, pixel_area=area, times=times[:, None])

    def route_a(o=o, d=d, area=area, ts=ts, te=te, ri=ri, rays=R, cand=cand):
        with torch.no_grad():
            return fld.render_packed(o, d, area, ts, te, ray_indices=ri, num_rays=rays, return_weights=True, actor_cand=cand)

    def route_b(rb=rb, o=o, d=d, ts=ts, te=te, ri=ri, rays=R):
        with torch.no_grad():
            rs = VolumetricSampler._gather(rb, o, d, ri, ts, te)
            out = fld(rs)
            res = render_packed(out[FieldHeadNames.FEATURE], rs, ri, rays, alpha=out[FieldHeadNames.ALPHA])
            return res["features"], res["depth"], res["accumulation"], res["weights"][:, 0]

    n = 1024
    m = int(seg[n])
    rb_s = RayBundle(origins=o[:n], directions=d[:n], pixel_area=area[:n], times=times[:n, None])
    sl = dict(o=o[:n].contiguous(), d=d[:n].contiguous(), ts=ts[:m], te=te[:m], ri=ri[:m], rays=n)
    got = route_a(area=area[:n], cand=tuple(None if c is None else c[:n].contiguous() for c in cand), **sl)
    want = route_b(rb=rb_s, **sl)
    agree = {k: rel_l2(x, y) for k, x, y in zip(("features", "depth", "accumulation", "weights"), got, want)}
    keys = ("a_fused_packed_actors", "b_gather_field_composite")
    lap = {k: [] for k in keys}
    for rep in range(args.warmup + args.reps):
        for key, fn in zip(keys, (route_a, route_b)):  # alternating
            t = timed(fn)
            if rep >= args.warmup:
                lap[key].append(t)
    med = {k: median(v) for k, v in lap.items()}
    line = {
        "bench": "render_packed_actors", "field": "neurad_default_8x4_h32", "levels": L, "features_per_level": F, "hidden": H,
        "log2_table": LOG2_T, "table_dtype": "fp32", "actors": A, "actor_grid": [cfg.grid.actor.num_levels, cfg.grid.actor.hashgrid_dim,
                                                                               cfg.grid.actor.log2_hashmap_size],
        "rays": R, "grid": RES, "occupancy": float(binaries.float().mean()), "step": STEP, "M": M, "M_plain_march": plain_m,
        "rays_with_candidates": float((cand[0] > 0).float().mean()), "max_candidates_on_a_ray": int(cand[0].max()),
        "segments": {"min": int(counts.min()), "median": float(np.median(counts)), "p99": float(np.percentile(counts, 99)),
                     "max": int(counts.max()), "empty_share": float((counts == 0).mean())},
        "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps, "warmup": args.warmup,
        "mlp_pairs": os.environ.get("NRHIP_MLP_PAIRS", "default"),
        "median_us": med, "min_us": {k: min(v) for k, v in lap.items()}, "max_us": {k: max(v) for k, v in lap.items()},
        "ratio_b_over_a": med[keys[1]] / med[keys[0]],
        "note": "march and per-ray candidate lists outside the timed region; (b) computes its own per-sample lists",
        "a_vs_b_rel_l2_1024_rays": agree,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    failed = [k for k, v in agree.items() if not v < TOL]
    if failed:
        raise SystemExit(f"bench_render_packed --actors: the two routes disagree on {failed}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", action="store_true", help="the fused packed-actors route against the operator route")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_render_packed.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_packed: no GPU")
    if args.actors:
        return main_actors(args)
    from bench import device_state

    clocks = device_state(0)
    gen = torch.Generator().manual_seed(0)
    binaries = (torch.rand((RES, RES, RES), generator=gen) < 0.3).cuda()
    o = ((torch.rand((R, 3), generator=gen) * 2 - 1) * 3.5).cuda()
    d = torch.nn.functional.normalize(torch.randn((R, 3), generator=gen), dim=-1).cuda()
    area = torch.full((R, 1), 2.4e-6, device="cuda")
    grid = ops.OccGridSpec(torch.tensor([-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]), binaries)
    ri, ts, te, seg = ops.occgrid_march(grid, o, d, STEP)
    M = int(ri.shape[0])
    counts = (seg[1:] - seg[:-1]).cpu().numpy()
    rb = RayBundle(origins=o, directions=d, pixel_area=area)
    n = 1024
    m = int(seg[n])
    failed = []
    for name, (L, F, H, base, max_res) in FIELDS.items():
        fld = make_field(L, F, H, base, max_res, gen)
        assert fld.fused_packed_supported()

        def route_a(o=o, d=d, area=area, ts=ts, te=te, ri=ri, rays=R):
            with torch.no_grad():
                return fld.render_packed(o, d, area, ts, te, ray_indices=ri, num_rays=rays, return_weights=True)

        def route_b(rb=rb, o=o, d=d, ts=ts, te=te, ri=ri, rays=R):
            with torch.no_grad():
                rs = VolumetricSampler._gather(rb, o, d, ri, ts, te)
                out = fld(rs)
                head = {"alpha": out[FieldHeadNames.ALPHA]} if fld.config.use_sdf else {"density": out[FieldHeadNames.DENSITY]}
                res = render_packed(out[FieldHeadNames.FEATURE], rs, ri, rays, **head)
                return res["features"], res["depth"], res["accumulation"], res["weights"][:, 0]

        # agreement on the first 1 024 rays, each route run on the slice alone
        rb_s = RayBundle(origins=o[:n], directions=d[:n], pixel_area=area[:n])
        sl = dict(o=o[:n].contiguous(), d=d[:n].contiguous(), ts=ts[:m], te=te[:m], ri=ri[:m], rays=n)
        got, want = route_a(area=area[:n], **sl), route_b(rb=rb_s, **sl)
        agree = {k: rel_l2(x, y) for k, x, y in zip(("features", "depth", "accumulation", "weights"), got, want)}
        times = {"a_fused_packed": [], "b_gather_field_composite": []}
        for rep in range(args.warmup + args.reps):
            for key, fn in (("a_fused_packed", route_a), ("b_gather_field_composite", route_b)):  # alternating
                t = timed(fn)
                if rep >= args.warmup:
                    times[key].append(t)
        med = {k: median(v) for k, v in times.items()}
        nbytes = M * (L * 8 * F * 4 + 8) + R * (40 + 136)
        line = {
            "bench": "render_packed", "field": name, "levels": L, "features_per_level": F, "hidden": H,
            "log2_table": LOG2_T, "table_dtype": "fp32", "rays": R, "grid": RES, "occupancy": float(binaries.float().mean()),
            "step": STEP, "M": M,
            "segments": {"min": int(counts.min()), "median": float(np.median(counts)), "p99": float(np.percentile(counts, 99)),
                         "max": int(counts.max()), "empty_share": float((counts == 0).mean())},
            "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps, "warmup": args.warmup,
            "mlp_pairs": os.environ.get("NRHIP_MLP_PAIRS", "default"),
            "median_us": med, "min_us": {k: min(v) for k, v in times.items()}, "max_us": {k: max(v) for k, v in times.items()},
            "ratio_b_over_a": med["b_gather_field_composite"] / med["a_fused_packed"],
            "a_whole_call": {"algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (med["a_fused_packed"] * 1e-6),
                             "share_of_8TBps_hbm_peak": nbytes / (med["a_fused_packed"] * 1e-6) / HBM_PEAK,
                             "note": "bytes from shapes (8 corner entries per level and sample, the interval, the per-ray "
                                     "constants and outputs) over the whole call's time (segments + kernel), not a kernel share"},
            "a_vs_b_rel_l2_1024_rays": agree,
        }
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line))
        failed += [f"{name}:{k}" for k, v in agree.items() if not v < TOL]
        del fld
        torch.cuda.empty_cache()
    if failed:
        raise SystemExit(f"bench_render_packed: the two routes disagree on {failed}")


if __name__ == "__main__":
    main()
