"""The chamfer distance of a lidar scan's evaluation at scan size: ops.chamfer_distance (csrc/lidar_eval.hip, brute force
through LDS tiles) against the formulation the reference runs (utils/math.py:745-798: 2 ceil(N / 1000) blocks of
torch.cdist(..., "use_mm_for_euclid_dist_if_necessary") with a row min and a sum each), written here in torch because the
reference tree is not on the GPU machine.  Two shapes: N = M = 2^17 and a ragged pair like a real scan (fewer predicted
returns than returned points).  Points lie inside +-80 x +-80 x +-4 m, the predictions a few decimetres off their targets.
The two legs alternate in one process, `--reps` repetitions after a warm-up, each timed with device events; the values of
the two legs are compared (the cdist form's cancellation error shows in the relative difference).  Appends ONE JSON line to
profiles/bench_lidar_eval.jsonl.  Fails without a GPU.
    python scripts/bench_lidar_eval.py [--reps 20] [--warmup 3] [--out profiles/bench_lidar_eval.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import device_state  # noqa: E402
from neurad_studio_amd import ops  # noqa: E402

SHAPES = {"pow2": (1 << 17, 1 << 17), "ragged": (97_531, 124_873)}


def chunked_cdist_chamfer(source, target, chunk=1_000):
    """the reference's formulation, normalised by the target count"""
    m = target.shape[0]
    s, t = source.view(1, -1, 3), target.view(1, -1, 3)
    total = torch.zeros((), device=source.device)
    for a, b in ((s, t), (t, s)):
        for i in range(0, a.shape[1], chunk):
            d = torch.cdist(a[:, i:i + chunk], b, p=2, compute_mode="use_mm_for_euclid_dist_if_necessary").pow(2)
            total += d.view(-1, b.shape[1]).min(dim=1).values.sum() / m
    return total


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out  # ms


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_lidar_eval.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lidar_eval: no GPU")
    clocks = device_state(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    box = torch.tensor([80.0, 80.0, 4.0], device="cuda")
    results = {}
    for name, (n, m) in SHAPES.items():
        target = (torch.rand((m, 3), device="cuda", generator=gen) * 2 - 1) * box
        pick = torch.randint(0, m, (n,), device="cuda", generator=gen)
        source = target[pick] + 0.3 * torch.randn((n, 3), device="cuda", generator=gen)
        legs = {"hip": lambda: ops.chamfer_distance(source, target, normalize_with_target=True),
                "cdist": lambda: chunked_cdist_chamfer(source, target)}
        times = {k: [] for k in legs}
        values = {}
        for rep in range(args.warmup + args.reps):
            for k, fn in legs.items():  # alternating in the same process
                ms, out = timed(fn)
                if rep >= args.warmup:
                    times[k].append(ms)
                values[k] = float(out)
        pairs = 2.0 * n * m
        results[name] = {"n": n, "m": m, "plan": list(ops.nearest_plan(n, m)), "plan_back": list(ops.nearest_plan(m, n)),
                         "median_ms": {k: median(v) for k, v in times.items()},
                         "min_max_ms": {k: [min(v), max(v)] for k, v in times.items()},
                         "value": values, "rel_diff_cdist_vs_hip": abs(values["cdist"] - values["hip"]) / values["hip"],
                         "hip_pairs_per_s": pairs / (median(times["hip"]) * 1e-3),
                         # 7 VALU operations per pair (3 sub, 1 mul, 2 fma, 1 min) = 9 flops with an fma as two
                         "hip_valu_tflops": 9.0 * pairs / (median(times["hip"]) * 1e-3) / 1e12,
                         "ratio_cdist_over_hip": median(times["cdist"]) / median(times["hip"])}
    line = {"bench": "lidar_eval_chamfer", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps,
            "warmup": args.warmup, "shapes": results,
            "note": "one call = both directions + the sum, device events around it (the hip leg includes its workspace "
                    "allocation; the cdist leg its 2 ceil(N / 1000) blocks with a [1000, M] temporary each); the tflops figure "
                    "is the whole call's rate, not a kernel's share of the 157 TF fp32 vector peak"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
