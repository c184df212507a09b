"""Median depth at the sizes a run meets: ops.median_depth / ops.median_depth_packed (csrc/median_depth.hip: one pass, one
wave per ray, left at the crossing) against the formulation the reference runs (model_components/renderers.py:387-397:
midpoints, cumsum, a constant tensor, searchsorted, clamp, gather -- six launches), written here in torch because the
reference tree is not on the GPU machine.  On a GPU torch.cumsum is an fp32 parallel scan, so the two legs agree on most rays,
not on all; the share that differs is recorded.

  dense_lidar     131072 x 32   a lidar scan's field samples
  dense_proposal   40960 x 128  a proposal round
  packed           65 536 rays marched through the occupancy grid of scripts/bench_render_packed.py's static scene.  The
                   reference has no packed median (renderers.py:390-391 raises): the baseline can only be a PADDED torch
                   formulation -- scatter the samples into [R, max count] (zero weights behind a ray's end), then the dense
                   one.  Both its whole time and the time without the padding are recorded.

Weights: alphas drawn so that most rays cross one half in their first quarter and some never do.  The legs alternate in one
process, `--reps` repetitions after a warm-up, each call timed with device events.  Appends ONE JSON line to
profiles/bench_median_depth.jsonl.  Fails without a GPU.
    python scripts/bench_median_depth.py [--reps 20] [--warmup 3] [--out profiles/bench_median_depth.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import device_state  # noqa: E402
from neurad_studio_amd import ops  # noqa: E402

DENSE = {"dense_lidar": (131072, 32), "dense_proposal": (40960, 128)}
PACKED_RAYS, RES, STEP = 65536, 128, 0.0125  # scripts/bench_render_packed.py's march


def torch_median(weights, starts, ends):
    """the reference's formulation on [R,S] tensors -> [R,1]"""
    steps = (starts + ends) / 2
    cumulative = torch.cumsum(weights, dim=-1)
    split = torch.ones((weights.shape[0], 1), device=weights.device) * 0.5
    index = torch.clamp(torch.searchsorted(cumulative, split, side="left"), 0, steps.shape[-1] - 1)
    return torch.gather(steps, dim=-1, index=index)


def pad(values, segments, ray_indices, width):
    """packed [M] -> [R, width], zeros behind a ray's end"""
    out = values.new_zeros((segments.shape[0] - 1, width))
    col = torch.arange(values.shape[0], device=values.device) - segments[ray_indices]
    out[ray_indices, col] = values
    return out


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
    stats = {"median_ms": {k: median(v) for k, v in times.items()}, "min_max_ms": {k: [min(v), max(v)] for k, v in times.items()}}
    return stats, outs


def alphas(shape, gen):
    """a ray's alphas: small, with a surface of a few opaque samples at a random place in its first half; every eighth ray
    has none (it never reaches one half)"""
    a = torch.rand(shape, device="cuda", generator=gen) * 0.02
    n = shape[-1]
    at = (torch.rand((shape[0], 1), device="cuda", generator=gen) * 0.5 * n).long()
    col = torch.arange(n, device="cuda")[None]
    hit = (col >= at) & (col < at + 3) & (torch.arange(shape[0], device="cuda")[:, None] % 8 != 0)
    return torch.where(hit, torch.full_like(a, 0.6), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_median_depth.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_median_depth: no GPU")
    clocks = device_state(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    results = {}
    for name, (R, S) in DENSE.items():
        edges = torch.sort(torch.rand((R, S + 1), device="cuda", generator=gen) * 100.0, dim=-1).values
        starts, ends = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
        w = ops.render_weight_from_alpha(alphas((R, S), gen))[0]
        stats, outs = run({"hip": lambda: ops.median_depth(w, starts, ends), "torch": lambda: torch_median(w, starts, ends)},
                          args.reps, args.warmup)
        _, idx = ops.median_depth(w, starts, ends, return_index=True)
        read = R * S * 4 + R * 8  # what the torch leg cannot avoid either: the weights once, two edges per ray
        results[name] = {"rays": R, "samples": S, **stats, "ratio_torch_over_hip": stats["median_ms"]["torch"] / stats["median_ms"]["hip"],
                         "share_of_rays_that_differ": float((outs["hip"] != outs["torch"]).float().mean()),
                         "mean_crossing_index": float(idx.float().mean()), "never_crossed_share": float((w.sum(-1) < 0.5).float().mean()),
                         "hip_GBps_of_full_weights": read / (stats["median_ms"]["hip"] * 1e-3) / 1e9}
    # packed: the march of bench_render_packed.py's static scene
    cpu = torch.Generator().manual_seed(0)
    binaries = (torch.rand((RES, RES, RES), generator=cpu) < 0.3).cuda()
    o = ((torch.rand((PACKED_RAYS, 3), generator=cpu) * 2 - 1) * 3.5).cuda()
    d = torch.nn.functional.normalize(torch.randn((PACKED_RAYS, 3), generator=cpu), dim=-1).cuda()
    grid = ops.OccGridSpec(torch.tensor([-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]), binaries)
    ri, ts, te, seg = ops.occgrid_march(grid, o, d, STEP)
    counts = seg[1:] - seg[:-1]
    width, M = int(counts.max()), int(ri.shape[0])
    a = torch.rand((M,), device="cuda", generator=gen) * 0.02
    a = torch.where(torch.rand((M,), device="cuda", generator=gen) < 0.02, torch.full_like(a, 0.6), a)
    w = ops.packed_weight_from_alpha(a, seg)[0]
    wp, sp, ep = (pad(v, seg, ri, width) for v in (w, ts, te))
    legs = {"hip": lambda: ops.median_depth_packed(w, ts, te, seg),
            "torch_padded": lambda: torch_median(*(pad(v, seg, ri, width) for v in (w, ts, te))),
            "torch_prepadded": lambda: torch_median(wp, sp, ep)}
    stats, outs = run(legs, args.reps, args.warmup)
    live = counts > 0
    results["packed"] = {"rays": PACKED_RAYS, "samples": M, "padded_width": width,
                         "segments": {"median": float(counts.float().median()), "max": width, "empty_share": float((~live).float().mean())},
                         **stats, "ratio_torch_padded_over_hip": stats["median_ms"]["torch_padded"] / stats["median_ms"]["hip"],
                         "ratio_torch_prepadded_over_hip": stats["median_ms"]["torch_prepadded"] / stats["median_ms"]["hip"],
                         # (a padded ray that never crosses lands on a padding sample; only rays that cross are compared)
                         "share_of_crossing_rays_that_differ": float(
                             (outs["hip"] != outs["torch_padded"])[(wp.sum(-1) >= 0.5)].float().mean())}
    line = {"bench": "median_depth", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps,
            "warmup": args.warmup, "shapes": results,
            "note": "whole calls, device events around each (the hip leg includes its output allocation; the torch leg its five "
                    "temporaries); the packed baseline is a padded torch formulation, the reference has none; GB/s counts the whole "
                    "weight array although the kernel leaves a ray at its crossing: a call's rate, not a share of the HBM peak"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
