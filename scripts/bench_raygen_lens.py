"""Ray generation at the c3 camera batch: 40 960 rays = 40 patches of 32 x 32 pixels drawn from six 3848 x 2168 cameras (the
cameras of tests/golden/raygen_lens.npz), rolling shutter on.  Two legs, alternating in one process, timed with device
events after a warm-up:
  lens   FISHEYE cameras with radial + tangential coefficients -> nrhip_camera_rays_lens (ten Newton iterations for each of
         the pixel and its two neighbours, then sinf / cosf);
  plain  the same cameras as undistorted PERSPECTIVE -> nrhip_camera_rays, the kernel every other dataset takes.
Each leg is timed twice: the bare entry point, `--launches` launches per timed window (one launch is a few microseconds,
less than an event pair resolves), and the whole `cameras.raygen.camera_rays` call with its allocations (20 per window),
which is what a training step pays.  Appends ONE JSON line to profiles/bench_raygen.jsonl.  The reference's op composition is not timed:
it is not on the GPU machine.  Fails without a GPU.
    python scripts/bench_raygen_lens.py [--reps 30] [--warmup 5] [--launches 200] [--out profiles/bench_raygen.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench import device_state  # noqa: E402
from neurad_studio_amd import _lib  # noqa: E402
from neurad_studio_amd.cameras import raygen  # noqa: E402
from neurad_studio_amd.ops import launch  # noqa: E402
from raygen_lens_cases import FISHEYE, PERSPECTIVE, H, W, cameras  # noqa: E402

PATCHES, K = 40, 32
R = PATCHES * K * K


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per call


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_raygen.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raygen_lens: no GPU")

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    clocks = device_state(0)
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "raygen_lens.npz")))
    C = g["c2w"].shape[0]
    gen = torch.Generator().manual_seed(0)
    cam = torch.randint(0, C, (PATCHES,), generator=gen)
    y0 = torch.randint(0, H - K + 1, (PATCHES,), generator=gen)
    x0 = torch.randint(0, W - K + 1, (PATCHES,), generator=gen)
    yy, xx = torch.meshgrid(torch.arange(K), torch.arange(K), indexing="ij")
    coords = torch.stack([(y0[:, None, None] + yy).float() + 0.5, (x0[:, None, None] + xx).float() + 0.5], -1).reshape(R, 2).cuda()
    idx = cam[:, None].expand(PATCHES, K * K).reshape(R, 1).contiguous().cuda()
    legs = {"lens": cameras(g, cuda, FISHEYE, distortion=True, rolling_shutter=True),
            "plain": cameras(g, cuda, PERSPECTIVE, distortion=False, rolling_shutter=True)}

    # the bare entry points on preallocated outputs
    tabs = {k: cuda(g[k].reshape(C, -1)) for k in ("c2w", "fx", "fy", "cx", "cy", "cam_times", "rolling_shutter_time",
                                                   "time_to_center_pixel", "cam_velocities", "distortion")}
    tabs["extent"] = torch.full((C, 1), float(H), device="cuda")
    t = _lib.CameraTable()
    (t.camera_to_worlds, t.fx, t.fy, t.cx, t.cy, t.times, t.rolling_shutter_time, t.time_to_center_pixel, t.velocities,
     t.shutter_extent) = (tabs[k].data_ptr() for k in ("c2w", "fx", "fy", "cx", "cy", "cam_times", "rolling_shutter_time",
                                                        "time_to_center_pixel", "cam_velocities", "extent"))
    t.rolling_shutter = 1
    lens = _lib.CameraLens()
    lens.camera_type, lens.distortion = FISHEYE, tabs["distortion"].data_ptr()
    outs = [torch.empty((R, n), device="cuda") for n in (3, 3, 1, 1, 1)]
    flat = idx.reshape(-1)
    runs = {"lens_entry": (lambda: launch("nrhip_camera_rays_lens", t, lens, flat, coords, R, *outs), args.launches),
            "plain_entry": (lambda: launch("nrhip_camera_rays", t, flat, coords, R, *outs), args.launches),
            "lens_call": (lambda: raygen.camera_rays(legs["lens"], idx, coords), 20),
            "plain_call": (lambda: raygen.camera_rays(legs["plain"], idx, coords), 20)}

    # the bare launch writes what the call returns (same tables), and the lens leg is finite
    rb = raygen.camera_rays(legs["lens"], idx, coords)
    runs["lens_entry"][0]()
    assert torch.equal(rb.directions, outs[1]) and torch.equal(rb.pixel_area, outs[2]) and bool(torch.isfinite(rb.directions).all())

    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for name, (fn, n) in runs.items():  # alternating in the same process
            us = window(fn, n)
            if rep >= args.warmup:
                times[name].append(us)
    med = {k: median(v) for k, v in times.items()}
    spread = {k: [min(v), max(v)] for k, v in times.items()}
    line = {"bench": "raygen_lens", "rays": R, "patches": PATCHES, "patch": K, "cameras": C, "image": [W, H],
            "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps, "warmup": args.warmup,
            "launches_per_window": args.launches, "median_us": med, "min_max_us": spread,
            "ratio_lens_over_plain": {k: med[f"lens_{k}"] / med[f"plain_{k}"] for k in ("entry", "call")},
            "note": "entry = back-to-back launches of the bare entry point (enqueue-bound when the kernel is shorter than a "
                    "launch); call = cameras.raygen.camera_rays with its allocations and metadata gathers"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
