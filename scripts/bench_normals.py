"""Surface normals at the sizes a run meets: the fused kernel (ops.field_normals / ops.field_normals_packed,
csrc/normals.hip) against the same result composed from the four operator kernels (ops.field_normals_operators: encode_fwd
-> mlp_fwd -> mlp_bwd of a unit cotangent -> encode_bwd_rays on [N,1] rays), and the cost of ``normals=True`` on the fused
eval chunk of the model.

  dense_40960x32     a camera batch's field samples
  dense_131072x32    a lidar scan's
  packed             65 536 rays marched through the occupancy grid of scripts/bench_render_packed.py's static scene; the operator
                     leg runs on the same samples as [M,1] rays (the ray constants gathered per sample outside the timing)
  eval_chunk         NeuRADHotPath.get_nff_outputs on 32 768 rays, with and without ``normals``

Field: NeuRAD's defaults (8 levels x 4 features on a 2^22 table, 32-wide MLPs, SDF head), the table scaled so that the
ReLUs are mixed.

--actors: a street of 32 moving boxes (two rows of 16) in the march's grid, NeuRAD's default actor grids (4 x 4 on 2^17 tables).
  dense_40960x32     40 960 rays x 32 samples through the street
  packed             65 536 rays through the box-aware march (ops.occgrid_march(..., actor_boxes=...))
Three legs each: the fused actor kernel (ops.field_normals(..., actors=...)), the operator composition
(ops.field_normals_operators(..., actors=...)) and the STATIC kernel on the same rays -- the price of the per-lane select.

The legs alternate in one process, `--reps` repetitions after a warm-up, each whole call between two device
events.  Appends ONE JSON line to profiles/bench_normals.jsonl.  Fails without a GPU.
    python scripts/bench_normals.py [--actors] [--reps 20] [--warmup 3] [--out profiles/bench_normals.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import device_state  # noqa: E402
from neurad_studio_amd import ops  # noqa: E402
from neurad_studio_amd.cameras.rays import RayBundle  # noqa: E402
from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig  # noqa: E402
from neurad_studio_amd.models.neurad import NeuRADHotPath, NeuRADHotPathConfig  # noqa: E402

DENSE = {"dense_40960x32": (40960, 32), "dense_131072x32": (131072, 32)}
PACKED_RAYS, RES, STEP = 65536, 128, 0.0125  # scripts/bench_render_packed.py's march
CHUNK = 32768
WANT = ("gradient", "normals")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out  # ms


def median(v):
    return sorted(v)[len(v) // 2]


def run(legs, reps, warmup):
    times, outs = {k: [] for k in legs}, {}
    for rep in range(warmup + reps):
        for k, fn in legs.items():  # alternating in the same process
            ms, outs[k] = timed(fn)
            if rep >= warmup:
                times[k].append(ms)
    return {"median_ms": {k: median(v) for k, v in times.items()}, "min_max_ms": {k: [min(v), max(v)] for k, v in times.items()}}, outs


def agreement(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def street(n_per_row=16):
    """two rows of boxes along x through the march's grid, moving 0.2 m between the two timestamps"""
    out = []
    for a in range(2 * n_per_row):
        row, k = divmod(a, n_per_row)
        p = torch.eye(4).repeat(2, 1, 1)
        p[:, :3, 3] = torch.tensor([-3.5 + 0.45 * k, -0.9 + 1.8 * row, -0.2 + 0.05 * (a % 3)])
        p[1, 0, 3] += 0.2
        out.append({"timestamps": torch.tensor([0.0, 1.0]), "poses": p, "dims": torch.tensor([0.2, 0.4, 0.16]),
                    "symmetric": torch.tensor(True), "deformable": torch.tensor(False)})
    return out


def main_actors(args):
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    clocks = device_state(0)
    cpu = torch.Generator().manual_seed(0)
    actors = DynamicActors(DynamicActorsConfig(actor_bbox_padding=(0.05, 0.05, 0.02)), trajectories=street())
    torch.manual_seed(0)
    fld = NeuRADField(NeuRADFieldConfig(), actors=actors, static_scale=4.0).cuda().eval()
    with torch.no_grad():
        for t in [fld.hashgrid.static_grid.hash_table] + [g.hash_table for g in fld.hashgrid.actor_grids]:
            t.copy_(((torch.rand(t.shape, generator=cpu) * 2 - 1) * 0.5).to(t.device))
    assert fld.normals_fused()
    fs = fld.field_spec()
    hg = fld.hashgrid
    o = ((torch.rand((PACKED_RAYS, 3), generator=cpu) * 2 - 1) * 3.5).cuda()
    d = torch.nn.functional.normalize(torch.randn((PACKED_RAYS, 3), generator=cpu), dim=-1).cuda()
    area = torch.full((PACKED_RAYS,), 2.4e-6, device="cuda")
    times = torch.rand((PACKED_RAYS,), generator=cpu).cuda()
    results = {}

    def three(name, fused, operators, static, extra):
        stats, outs = run({"fused_actors": fused, "operators_actors": operators, "static_kernel_same_rays": static},
                          args.reps, args.warmup)
        hit = outs["fused_actors"]["hit"].reshape(-1)
        med = stats["median_ms"]
        results[name] = {**extra, **stats, "in_box_share": float((hit >= 0).float().mean()),
                         "ratio_operators_over_fused": med["operators_actors"] / med["fused_actors"],
                         "ratio_fused_actors_over_static": med["fused_actors"] / med["static_kernel_same_rays"],
                         "rel_l2_gradient_fused_vs_operators": {
                             k: agreement(outs["fused_actors"]["gradient"].reshape(-1, 3)[m],
                                          outs["operators_actors"]["gradient"].reshape(-1, 3)[m])
                             for k, m in (("in_a_box", hit >= 0), ("outside", hit < 0))}}

    # dense: 40 960 of the rays, 32 samples each across the grid
    R, S = DENSE["dense_40960x32"]
    gen = torch.Generator(device="cuda").manual_seed(0)
    edges = torch.sort(torch.rand((R, S + 1), device="cuda", generator=gen) * 7.0, dim=-1).values
    starts, ends = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
    oR, dR, aR, tR = o[:R].contiguous(), d[:R].contiguous(), area[:R].contiguous(), times[:R].contiguous()
    spec, cand = hg.prepare_actors(oR, dR, aR, starts, ends, tR)
    three("dense_40960x32",
          lambda: ops.field_normals(fs, oR, dR, aR, starts, ends, want=WANT + ("hit",), actors=(spec, cand)),
          lambda: ops.field_normals_operators(fs, oR, dR, aR, starts, ends, want=WANT, actors=(spec, cand), times=tR),
          lambda: ops.field_normals(fs, oR, dR, aR, starts, ends, want=WANT),
          {"rays": R, "samples": S, "rays_with_candidates": float((cand[0] > 0).float().mean())})
    # packed: the box-aware march; the operator leg on the same samples as [M,1] rays, the ray constants and the candidate
    # lists gathered per sample outside the timing
    binaries = (torch.rand((RES, RES, RES), generator=cpu) < 0.3).cuda()
    grid = ops.OccGridSpec(torch.tensor([-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]), binaries)
    spec, cand = hg.prepare_actors_line(o, d, 0.0, 1.0, times)
    ri, ts, te, seg = ops.occgrid_march(grid, o, d, STEP, actor_boxes=(spec, cand))
    M = int(ri.shape[0])
    o1, d1, a1, t1, s1, e1 = o[ri], d[ri], area[ri], times[ri], ts.reshape(M, 1), te.reshape(M, 1)
    cand1 = tuple(None if c is None else c[ri].contiguous() for c in cand)
    counts = seg[1:] - seg[:-1]
    three("packed",
          lambda: ops.field_normals_packed(fs, o, d, area, ts, te, seg, want=WANT + ("hit",), actors=(spec, cand)),
          lambda: ops.field_normals_operators(fs, o1, d1, a1, s1, e1, want=WANT, actors=(spec, cand1), times=t1),
          lambda: ops.field_normals_packed(fs, o, d, area, ts, te, seg, want=WANT),
          {"rays": PACKED_RAYS, "samples": M, "segments": {"median": float(counts.float().median()), "max": int(counts.max())}})
    line = {"bench": "normals_actors", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps,
            "warmup": args.warmup, "actors": int(actors.n_actors),
            "field": "8 x 4 levels on a 2^22 fp32 table, H = 32, SDF head; actor grids 4 x 4 on 2^17 fp32 tables", "shapes": results,
            "note": "one box, measured once; whole calls between device events, candidate lists and the march outside them "
                    "(each leg includes its output allocations; the operator leg its temporaries, one host read of the in-box "
                    "count and the torch glue between its kernels)"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", action="store_true", help="the actor-aware kernel, the operator composition and the static kernel")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_normals.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals: no GPU")
    if args.actors:
        return main_actors(args)
    clocks = device_state(0)
    torch.manual_seed(0)
    fld = NeuRADField(NeuRADFieldConfig(), actors=None, static_scale=100.0).cuda().eval()
    with torch.no_grad():
        fld.hashgrid.static_grid.hash_table.mul_(1000.0)
    fs = fld.field_spec()
    gen = torch.Generator(device="cuda").manual_seed(0)
    results = {}
    for name, (R, S) in DENSE.items():
        o = (torch.rand((R, 3), device="cuda", generator=gen) * 2 - 1) * 20.0
        d = torch.nn.functional.normalize(torch.randn((R, 3), device="cuda", generator=gen), dim=-1)
        area = torch.full((R,), 2.7e-7, device="cuda")
        edges = torch.sort(torch.rand((R, S + 1), device="cuda", generator=gen) ** 2 * 300.0, dim=-1).values
        starts, ends = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
        w = torch.rand((R, S), device="cuda", generator=gen)
        legs = {"fused": lambda: ops.field_normals(fs, o, d, area, starts, ends, want=WANT),
                "operators": lambda: ops.field_normals_operators(fs, o, d, area, starts, ends, want=WANT),
                "fused_ray_sum_only": lambda: ops.field_normals(fs, o, d, area, starts, ends, weights=w, want=("ray_normals",))}
        stats, outs = run(legs, args.reps, args.warmup)
        results[name] = {"rays": R, "samples": S, **stats,
                         "ratio_operators_over_fused": stats["median_ms"]["operators"] / stats["median_ms"]["fused"],
                         "rel_l2_gradient_fused_vs_operators": agreement(outs["fused"]["gradient"], outs["operators"]["gradient"])}
    # packed: the march of bench_render_packed.py's static scene
    cpu = torch.Generator().manual_seed(0)
    binaries = (torch.rand((RES, RES, RES), generator=cpu) < 0.3).cuda()
    o = ((torch.rand((PACKED_RAYS, 3), generator=cpu) * 2 - 1) * 3.5).cuda()
    d = torch.nn.functional.normalize(torch.randn((PACKED_RAYS, 3), generator=cpu), dim=-1).cuda()
    area = torch.full((PACKED_RAYS,), 2.7e-7, device="cuda")
    grid = ops.OccGridSpec(torch.tensor([-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]), binaries)
    ri, ts, te, seg = ops.occgrid_march(grid, o, d, STEP)
    M = int(ri.shape[0])
    o1, d1, a1, s1, e1 = o[ri], d[ri], area[ri], ts.reshape(M, 1), te.reshape(M, 1)
    legs = {"fused": lambda: ops.field_normals_packed(fs, o, d, area, ts, te, seg, want=WANT),
            "operators": lambda: ops.field_normals_operators(fs, o1, d1, a1, s1, e1, want=WANT)}
    stats, outs = run(legs, args.reps, args.warmup)
    counts = seg[1:] - seg[:-1]
    results["packed"] = {"rays": PACKED_RAYS, "samples": M,
                         "segments": {"median": float(counts.float().median()), "max": int(counts.max())}, **stats,
                         "ratio_operators_over_fused": stats["median_ms"]["operators"] / stats["median_ms"]["fused"],
                         "rel_l2_gradient_fused_vs_operators": agreement(outs["fused"]["gradient"],
                                                                         outs["operators"]["gradient"].reshape(M, 3))}
    # the eval chunk with and without the normals
    c = NeuRADHotPathConfig(appearance_dim=0)
    c.field.sdf_beta = 3.0
    torch.manual_seed(0)
    m = NeuRADHotPath(c, static_scale=100.0).cuda().eval()
    with torch.no_grad():
        m.field.hashgrid.static_grid.hash_table.mul_(1000.0)
        for p in m.proposal_fields:
            p.hashgrid.static_grid.hash_table.mul_(2000.0)
    ro = (torch.rand((CHUNK, 3), device="cuda", generator=gen) * 2 - 1) * 20.0
    rd = torch.nn.functional.normalize(torch.randn((CHUNK, 3), device="cuda", generator=gen), dim=-1)

    def chunk(flag):
        m.normals = flag
        rb = RayBundle(origins=ro, directions=rd, pixel_area=torch.full((CHUNK, 1), 2.7e-7, device="cuda"),
                       nears=torch.zeros(CHUNK, 1, device="cuda"), fars=torch.full((CHUNK, 1), 20000.0, device="cuda"))
        with torch.no_grad():
            return m.get_nff_outputs(rb)

    stats, outs = run({"without": lambda: chunk(False), "with_normals": lambda: chunk(True)}, args.reps, args.warmup)
    results["eval_chunk"] = {"rays": CHUNK, **stats,
                             "added_ms": stats["median_ms"]["with_normals"] - stats["median_ms"]["without"],
                             "ratio_with_over_without": stats["median_ms"]["with_normals"] / stats["median_ms"]["without"],
                             "has_key": "normals" in outs["with_normals"] and "normals" not in outs["without"]}
    line = {"bench": "normals", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps, "warmup": args.warmup,
            "field": "8 x 4 levels on a 2^22 fp32 table, H = 32, SDF head", "shapes": results,
            "note": "one box, measured once; whole calls between device events (each leg includes its output allocations; the "
                    "operator leg its [N, L*F] temporaries, the weight-gradient buffers of mlp_bwd and the torch normalisation)"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
