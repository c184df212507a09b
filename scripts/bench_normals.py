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
ReLUs are mixed.  The legs alternate in one process, `--reps` repetitions after a warm-up, each whole call between two device
events.  Appends ONE JSON line to profiles/bench_normals.jsonl.  Fails without a GPU.
    python scripts/bench_normals.py [--reps 20] [--warmup 3] [--out profiles/bench_normals.jsonl]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_normals.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals: no GPU")
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
