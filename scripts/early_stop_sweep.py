"""Headline render kernel: time against tiles actually run, at several early_stop_eps (0 = every tile).
usage: python scripts/early_stop_sweep.py [out.json]   (NEURAD_HIP_LIB selects the library)
A tile counts as run when it lies at or before the ray's last non-zero weight (a skipped tile's weights are written 0)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from neurad_studio_amd import ops  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    fs, o, d, area, fars = bench.make_workload(dev, seed=1234)
    S = bench.N_SAMPLES
    _, eu, order = ops.power_sampler_ordered(None, fars, S, o, d, bench.STATIC_SCALE, lam=-1.0, scaling=0.1, last_edge=20000.0)
    s0, s1 = eu[:, :-1], eu[:, 1:]
    rows = []
    for eps in (0.0, 1e-6, 1e-4, 1e-2, 0.1, 0.5):
        w = ops.render_fwd(fs, o, d, area, s0, s1, return_weights=True, early_stop_eps=eps, order=order)[3]
        nz = (w != 0).reshape(w.shape[0], -1, 16).any(-1)  # [R, tiles]
        last = torch.where(nz.any(-1), nz.shape[1] - 1 - nz.flip(-1).float().argmax(-1), torch.zeros_like(nz[:, 0], dtype=torch.long))
        tiles = int((last + 1).sum())
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for k in range(25):
            if k >= 5:
                evs[k - 5][0].record()
            ops.render_fwd(fs, o, d, area, s0, s1, early_stop_eps=eps, order=order)
            if k >= 5:
                evs[k - 5][1].record()
        torch.cuda.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in evs]
        rows.append({"early_stop_eps": eps, "tiles_run": tiles, "tiles_per_ray": tiles / w.shape[0],
                     "kernel_us_median": float(np.median(us)), "kernel_us_min": float(np.min(us))})
        print(rows[-1], flush=True)
    if len(sys.argv) > 1:
        json.dump({"what": "render_kernel<16,2,64,fp32,composite,pairs> on the c1 batch, HIP events around 20 launches",
                   "library": os.environ.get("NEURAD_HIP_LIB", "default"), "rows": rows}, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
