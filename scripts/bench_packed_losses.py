"""The two per-sample loss terms on packed, occupancy-marched samples: ops.packed_distortion_loss_rays and
ops.packed_lidar_carving (csrc/losses.hip: one wave per ray, O(n) per ray, value and gradient in one launch) against the
only formulation there was before them: scatter the samples into [R, max count] (zero weights behind a ray's end) and

  carving      run the dense kernel (ops.lidar_carving) on the padded tensors, gather the gradient back to [M];
  distortion   the dense kernel (ops.distortion_loss_rays) takes CONTIGUOUS edges [R,S+1] and at most 512 samples: a marched
               ray has gaps, so it cannot give this value at any width.  The baseline is the reference's O(n^2) expression
               (model_components/losses.py:137-148,159-200) in torch on the padded tensors, rays in slabs so that the
               [rays, S, S] temporary fits, value and gradient from the one inner sum.  Where the width allows it the dense
               kernel is timed too, on the padded starts as if they were contiguous edges: a time, not the same value.

  marched   65 536 rays through the occupancy grid of scripts/bench_render_packed.py's static scene (about 6 M samples)
  lidar     16 384 of those rays as one lidar batch (two thirds returned)

Each leg's whole time and, for the baselines, the time without the padding are recorded.  The legs alternate in one process,
`--reps` repetitions after a warm-up, each call under device events.  Appends ONE JSON line per size to
profiles/bench_packed_losses.jsonl.  Fails without a GPU.
    python scripts/bench_packed_losses.py [--reps 20] [--warmup 3] [--out profiles/bench_packed_losses.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import device_state  # noqa: E402
from neurad_studio_amd import ops  # noqa: E402

SIZES = {"marched": 65536, "lidar": 16384}
RES, STEP = 128, 0.0125  # scripts/bench_render_packed.py's march
EPS, NON_RETURN = 0.1, 6.0
SLAB_BYTES = 1 << 30  # the O(n^2) baseline's [rays, S, S] fp32 temporary


def pad(values, segments, ray_indices, width):
    """packed [M] -> [R, width], zeros behind a ray's end"""
    out = values.new_zeros((segments.shape[0] - 1, width))
    col = torch.arange(values.shape[0], device=values.device) - segments[ray_indices]
    out[ray_indices, col] = values
    return out


def unpad(padded, segments, ray_indices):
    col = torch.arange(ray_indices.shape[0], device=padded.device) - segments[ray_indices]
    return padded[ray_indices, col]


def torch_distortion(w, s, e):
    """the reference's expression on padded [R,S] tensors -> loss [R], d loss / d w [R,S]; rays in slabs"""
    R, S = w.shape
    slab = max(1, SLAB_BYTES // (S * S * 4))
    loss, grad = w.new_empty((R,)), torch.empty_like(w)
    for b in range(0, R, slab):
        ws, m, d = w[b:b + slab], (s[b:b + slab] + e[b:b + slab]) / 2, e[b:b + slab] - s[b:b + slab]
        inner = (ws[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum(-1)  # sum_j w_j |m_i - m_j|
        loss[b:b + slab] = (ws * inner).sum(-1) + (ws * ws * d).sum(-1) / 3
        grad[b:b + slab] = 2 * inner + (2.0 / 3.0) * ws * d
    return loss, grad


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


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def one_size(name, R, o, d, grid, gen, reps, warmup):
    ri, ts, te, seg = ops.occgrid_march(grid, o[:R].contiguous(), d[:R].contiguous(), STEP)
    counts = seg[1:] - seg[:-1]
    width, M = int(counts.max()), int(ri.shape[0])
    a = torch.rand((M,), device="cuda", generator=gen) * 0.02
    a = torch.where(torch.rand((M,), device="cuda", generator=gen) < 0.02, torch.full_like(a, 0.6), a)
    w = ops.packed_weight_from_alpha(a, seg)[0]
    # a lidar batch: every ray a beam, two thirds returned, at the depth the weights put the surface (so that some samples
    # are close to it); the marched size keeps two thirds of its rays as camera rays
    ray = torch.arange(R, device="cuda")
    is_lidar = (ray % 3 == 0) if name == "marched" else torch.ones(R, dtype=torch.bool, device="cuda")
    did_return = ray % 3 != 1
    distance = ops.packed_accumulate(w, ((ts + te) / 2)[:, None].contiguous(), seg)[:, 0].contiguous()
    carve = (is_lidar, did_return, distance, EPS, NON_RETURN)
    wp, sp, ep = (pad(v, seg, ri, width) for v in (w, ts, te))

    def carving_padded(pre):
        p = (wp, sp, ep) if pre else tuple(pad(v, seg, ri, width) for v in (w, ts, te))
        _, loss, g = ops.lidar_carving(p[1], p[2], *carve, weights=p[0], want_mask=False)
        return loss, (g if pre else unpad(g, seg, ri))

    def distortion_padded(pre):
        p = (wp, sp, ep) if pre else tuple(pad(v, seg, ri, width) for v in (w, ts, te))
        loss, g = torch_distortion(*p)
        return loss, (g if pre else unpad(g, seg, ri))

    legs = {"hip_distortion": lambda: ops.packed_distortion_loss_rays(ts, te, w, seg),
            "torch_distortion_padded": lambda: distortion_padded(False),
            "torch_distortion_prepadded": lambda: distortion_padded(True),
            "hip_carving": lambda: ops.packed_lidar_carving(ts, te, seg, *carve, weights=w, want_mask=False)[1:],
            "dense_carving_padded": lambda: carving_padded(False),
            "dense_carving_prepadded": lambda: carving_padded(True)}
    if width <= 512:  # the dense distortion kernel on the padded starts as contiguous edges: a time, not the same value
        edges = torch.cat([sp, ep[:, -1:]], -1).contiguous()
        legs["dense_distortion_kernel_on_prepadded_edges"] = lambda: ops.distortion_loss_rays(edges, wp)
    stats, outs = run(legs, reps, warmup)
    t = stats["median_ms"]
    read = 3 * M * 4 + (R + 1) * 8
    return {"bench": "packed_losses", "size": name, "rays": R, "samples": M, "padded_width": width,
            "segments": {"median": float(counts.float().median()), "max": width,
                         "empty_share": float((counts == 0).float().mean())},
            "lidar_rays": int(is_lidar.sum()), **stats,
            "ratio_distortion_padded_over_hip": t["torch_distortion_padded"] / t["hip_distortion"],
            "ratio_distortion_prepadded_over_hip": t["torch_distortion_prepadded"] / t["hip_distortion"],
            "ratio_carving_padded_over_hip": t["dense_carving_padded"] / t["hip_carving"],
            "ratio_carving_prepadded_over_hip": t["dense_carving_prepadded"] / t["hip_carving"],
            "hip_distortion_GBps": (read + M * 4 + R * 4) / (t["hip_distortion"] * 1e-3) / 1e9,
            "hip_carving_GBps": (read + M * 4 + R * 4) / (t["hip_carving"] * 1e-3) / 1e9,
            "distortion_loss_rel_diff_vs_torch_fp32": rel(outs["hip_distortion"][0], outs["torch_distortion_padded"][0]),
            "distortion_grad_rel_diff_vs_torch_fp32": rel(outs["hip_distortion"][1], outs["torch_distortion_padded"][1]),
            "carving_loss_rel_diff_vs_dense": rel(outs["hip_carving"][0], outs["dense_carving_padded"][0]),
            "carving_grad_equal_to_dense": bool(torch.equal(outs["hip_carving"][1], outs["dense_carving_padded"][1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_packed_losses.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_packed_losses: no GPU")
    clocks = device_state(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    cpu = torch.Generator().manual_seed(0)
    binaries = (torch.rand((RES, RES, RES), generator=cpu) < 0.3).cuda()
    n = max(SIZES.values())
    o = ((torch.rand((n, 3), generator=cpu) * 2 - 1) * 3.5).cuda()
    d = torch.nn.functional.normalize(torch.randn((n, 3), generator=cpu), dim=-1).cuda()
    grid = ops.OccGridSpec(torch.tensor([-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]), binaries)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name, R in SIZES.items():
        line = {**one_size(name, R, o, d, grid, gen, args.reps, args.warmup), "device": torch.cuda.get_device_name(0),
                "clocks": clocks, "reps": args.reps, "warmup": args.warmup,
                "note": "whole calls, device events around each (every leg includes its output allocations; value and gradient "
                        "from each); *_padded legs scatter the three [M] arrays into [R, max count] and gather the gradient back, "
                        "*_prepadded legs start from padded tensors and leave the gradient padded; GB/s counts the three inputs "
                        "once and the two outputs: a call's rate (the distortion gradient of rays longer than 64 samples walks "
                        "the inputs twice)"}
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line))


if __name__ == "__main__":
    main()
