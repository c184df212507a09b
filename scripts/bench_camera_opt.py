"""Camera pose correction at batch size: forward + backward of autograd.PoseApplyFn (csrc/pose_opt.hip: one launch forwards;
clear, per-camera max, integer accumulate and finish backwards) against the reference's op sequence restated in torch on the
same GPU (index the parameter, the exponential map with its strided index assignments, two bmm; autograd's own backward ending
in the index backward into [C, 6]).  Batch: 40 960 patch-ordered rays (runs of 1024 per camera) followed by 16 384 rays with
uniformly random camera indices, C = 560 cameras.  The backward alone is also timed for the patch-ordered and the random part
separately (the two shapes of atomics: one row of adds per wave, four rows per wave-instruction).  The legs alternate in one
process, `--reps` repetitions after a warm-up, each timed with device events around the whole call (allocations included).
Kernel launches per route are counted in a separate pass with torch's profiler.  Appends ONE JSON line to
profiles/bench_camera_opt.jsonl.  Fails without a GPU.
    python scripts/bench_camera_opt.py [--reps 20] [--warmup 5] [--out profiles/bench_camera_opt.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import device_state  # noqa: E402
from neurad_studio_amd import ops  # noqa: E402
from neurad_studio_amd.autograd import PoseApplyFn  # noqa: E402

N_PATCH_RAYS, PATCH, N_RANDOM_RAYS, N_CAMERAS = 40960, 1024, 16384, 560


def torch_route(pose, idx, o, d):
    """the reference's sequence of torch ops (cameras/lie_groups.py:35-58, cameras/camera_optimizers.py:173-182)"""
    tv = pose[idx, :]
    w = tv[:, 3:]
    nrms = (w * w).sum(1)
    ang = torch.clamp(nrms, 1e-4).sqrt()
    inv = 1.0 / ang
    f1 = inv * ang.sin()
    f2 = inv * inv * (1.0 - ang.cos())
    K = torch.zeros((w.shape[0], 3, 3), dtype=w.dtype, device=w.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    m = torch.zeros(tv.shape[0], 3, 4, dtype=tv.dtype, device=tv.device)
    m[:, :3, :3] = f1[:, None, None] * K + f2[:, None, None] * torch.bmm(K, K) + torch.eye(3, dtype=w.dtype, device=w.device)[None]
    m[:, :3, 3] = tv[:, :3]
    return o + m[:, :3, 3], torch.bmm(m[:, :3, :3], d[..., None]).squeeze().to(o)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out  # ms


def median(v):
    return sorted(v)[len(v) // 2]


def launches(fn):
    """device kernels (memsets and copies included) one call enqueues, from torch's profiler; an error string where it fails"""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:  # noqa: BLE001
        return f"{type(e).__name__}: {e}"[:200]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_camera_opt.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_opt: no GPU")
    clocks = device_state(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)  # noqa: E731
    R = N_PATCH_RAYS + N_RANDOM_RAYS
    patch_cams = torch.randint(0, N_CAMERAS, (N_PATCH_RAYS // PATCH,), device="cuda", generator=gen)
    idx = torch.cat([patch_cams.repeat_interleave(PATCH), torch.randint(0, N_CAMERAS, (N_RANDOM_RAYS,), device="cuda", generator=gen)])
    pose = (rn(N_CAMERAS, 6) * 0.02).requires_grad_(True)
    o, d = rn(R, 3) * 50.0, torch.nn.functional.normalize(rn(R, 3), dim=1)
    g_o, g_d = rn(R, 3), rn(R, 3) * 30.0
    parts = {"all": slice(0, R), "patch_ordered": slice(0, N_PATCH_RAYS), "random": slice(N_PATCH_RAYS, R)}

    def node_step():
        o2, d2 = PoseApplyFn.apply(pose, None, idx, o, d)
        return torch.autograd.grad([o2, d2], [pose], [g_o, g_d])[0]

    def torch_step():
        o2, d2 = torch_route(pose, idx, o, d)
        return torch.autograd.grad([o2, d2], [pose], [g_o, g_d])[0]

    legs = {"step": {"hip": node_step, "torch": torch_step}}
    for name, sl in parts.items():
        i, dd, go, gd = idx[sl].contiguous(), d[sl].contiguous(), g_o[sl].contiguous(), g_d[sl].contiguous()
        oo = o[sl].contiguous()
        t_out = torch_route(pose, i, oo, dd)
        legs[f"backward_{name}"] = {
            "hip": lambda i=i, dd=dd, go=go, gd=gd: ops.pose_apply_bwd(pose.detach(), None, i, dd, go, gd)[0],
            "torch": lambda t_out=t_out, go=go, gd=gd: torch.autograd.grad(list(t_out), [pose], [go, gd], retain_graph=True)[0]}
    results = {}
    for what, pair in legs.items():
        times = {k: [] for k in pair}
        last = {}
        for rep in range(args.warmup + args.reps):
            for k, fn in pair.items():  # alternating in the same process
                ms, out = timed(fn)
                if rep >= args.warmup:
                    times[k].append(ms)
                last[k] = out
        diff = (last["hip"].double() - last["torch"].double()).norm() / last["torch"].double().norm()
        results[what] = {"median_ms": {k: median(v) for k, v in times.items()},
                         "min_max_ms": {k: [min(v), max(v)] for k, v in times.items()},
                         "ratio_torch_over_hip": median(times["torch"]) / median(times["hip"]),
                         "grad_rel_l2_hip_vs_torch_fp32": float(diff)}
    counts = {what: {k: launches(fn) for k, fn in pair.items()} for what, pair in legs.items() if what in ("step", "backward_all")}
    line = {"bench": "camera_opt_pose_apply", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps,
            "warmup": args.warmup, "rays": {"patch_ordered": N_PATCH_RAYS, "patch": PATCH, "random": N_RANDOM_RAYS},
            "cameras": N_CAMERAS, "results": results, "device_launches": counts,
            "atomic_bytes": {"patch_ordered": N_PATCH_RAYS // 64 * 96, "random": N_RANDOM_RAYS * 96},
            "note": "one call = forward + backward to the [C, 6] parameter gradient (step) or the backward alone, device events "
                    "around it, allocations included.  hip: autograd.PoseApplyFn / ops.pose_apply_bwd (csrc/pose_opt.hip; 64-bit "
                    "integer atomic adds, 96 bytes per uniform wave or per ray of a mixed wave).  torch: the reference's op "
                    "sequence restated in torch, fp32, no autocast.  device_launches: kernels, memsets and copies torch's "
                    "profiler lists for one call"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
