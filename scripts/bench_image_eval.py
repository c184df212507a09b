"""PSNR and SSIM of a camera image's evaluation at image size: model_components/image_metrics.py:image_eval_metrics
(csrc/image_eval.hip: two passes, one device->host transfer for the two scalars) against torchmetrics' algorithm restated
in torch, fp32, on the same GPU (reflect pad, one 15-channel grouped conv2d over the five product images, crop; two min / max
reductions; PSNR as a mean; a ``float()`` per metric, as models/neurad.py:585-586 pays them).  torchmetrics ITSELF is not
installed on these machines: the second leg is its algorithm, not its code.  Two shapes: 1080 x 1920 x 3 and 900 x 1600 x 3
(a smooth image and itself plus 2 % noise).  The two legs alternate in one process, `--reps` repetitions after a warm-up,
each timed with device events around the whole call (host reads included).  Also reported: the bytes the kernels request
against the 2 x image size the problem needs, and the tile amplification ((T + 10) / T)^2 of the SSIM pass.  Appends ONE JSON
line to profiles/bench_image_eval.jsonl.  Fails without a GPU.
    python scripts/bench_image_eval.py [--reps 20] [--warmup 5] [--out profiles/bench_image_eval.jsonl]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import device_state  # noqa: E402
from neurad_studio_amd import ops  # noqa: E402
from neurad_studio_amd.model_components.image_metrics import gaussian_window, image_eval_metrics  # noqa: E402

SHAPES = {"1080p": (1080, 1920, 3), "900x1600": (900, 1600, 3)}
WINDOW, PAD = 11, 5


def torchmetrics_form(image, rgb, kernel):
    """[H,W,3] fp32 device tensors -> (psnr, ssim) Python floats, the way the reference gets them"""
    p, t = torch.moveaxis(image, -1, 0)[None], torch.moveaxis(rgb, -1, 0)[None]
    psnr = float(10.0 * torch.log10(1.0 / torch.mean((p - t) ** 2)))
    r = torch.maximum(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * r) ** 2, (0.03 * r) ** 2
    pp = torch.nn.functional.pad(p, (PAD, PAD, PAD, PAD), mode="reflect")
    tp = torch.nn.functional.pad(t, (PAD, PAD, PAD, PAD), mode="reflect")
    out = torch.nn.functional.conv2d(torch.cat([pp, tp, pp * pp, tp * tp, pp * tp]), kernel, groups=p.shape[1])
    mu_p, mu_t, e_pp, e_tt, e_pt = (out[i:i + 1] for i in range(5))
    mu_pp, mu_tt, mu_pt = mu_p * mu_p, mu_t * mu_t, mu_p * mu_t
    var_p, var_t, cov = torch.clamp(e_pp - mu_pp, min=0.0), torch.clamp(e_tt - mu_tt, min=0.0), e_pt - mu_pt
    full = ((2 * mu_pt + c1) * (2 * cov + c2)) / ((mu_pp + mu_tt + c1) * (var_p + var_t + c2))
    return psnr, float(full[..., PAD:-PAD, PAD:-PAD].mean())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out  # ms


def median(v):
    return sorted(v)[len(v) // 2]


def requested_bytes(h, w, c, tile):
    """what the two passes ask the memory system for: both images once, then every tile's halo inside the image, per channel"""
    halo = 0
    for y0 in range(0, h - WINDOW + 1, tile):
        for x0 in range(0, w - WINDOW + 1, tile):
            halo += (min(y0 + tile + WINDOW - 1, h) - y0) * (min(x0 + tile + WINDOW - 1, w) - x0)
    return 2 * 4 * h * w * c + 2 * 4 * halo * c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_image_eval.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_eval: no GPU")
    clocks = device_state(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    g = gaussian_window(torch.float32, "cuda")
    kernel = (g[:, None] * g[None, :]).expand(3, 1, WINDOW, WINDOW).contiguous()
    tile = ops.SSIM_TILE
    results = {}
    for name, (h, w, c) in SHAPES.items():
        y, x = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
        ch = torch.arange(c, device="cuda")
        image = 0.5 + 0.4 * torch.sin(2 * math.pi * (y[..., None] / 137.0 + x[..., None] / 211.0) + 0.7 * ch)
        rgb = (image + 0.02 * torch.randn((h, w, c), device="cuda", generator=gen)).contiguous()
        image = image.contiguous()
        legs = {"hip": lambda: tuple(image_eval_metrics(rgb, image).values()),
                "torch_fp32": lambda: torchmetrics_form(image, rgb, kernel)}
        times = {k: [] for k in legs}
        values = {}
        for rep in range(args.warmup + args.reps):
            for k, fn in legs.items():  # alternating in the same process
                ms, out = timed(fn)
                if rep >= args.warmup:
                    times[k].append(ms)
                values[k] = list(out)
        needed = 2 * 4 * h * w * c
        results[name] = {"shape": [h, w, c],
                         "median_ms": {k: median(v) for k, v in times.items()},
                         "min_max_ms": {k: [min(v), max(v)] for k, v in times.items()},
                         "psnr_ssim": values,
                         "ssim_diff_torch_fp32_minus_hip": values["torch_fp32"][1] - values["hip"][1],
                         "bytes_needed": needed, "bytes_requested": requested_bytes(h, w, c, tile),
                         "requested_over_needed": requested_bytes(h, w, c, tile) / needed,
                         "tile_amplification": ((tile + WINDOW - 1) / tile) ** 2,
                         "ratio_torch_over_hip": median(times["torch_fp32"]) / median(times["hip"])}
    line = {"bench": "image_eval_psnr_ssim", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps,
            "warmup": args.warmup, "tile": tile, "shapes": results,
            "note": "one call = both metrics as Python floats, device events around it: the hip leg is image_eval_metrics "
                    "(workspace allocation, four launches, ONE device->host read); the torch_fp32 leg is torchmetrics' "
                    "ALGORITHM restated in torch (torchmetrics itself is not installed here), newer-version variance clamp, "
                    "with the reference's float() per metric.  bytes_requested counts every halo read of pass 2, most of "
                    "which the caches serve; it is not a DRAM traffic measurement"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
