"""LPIPS of one camera image against its ground truth, the whole ``LPIPS.forward`` call (model_components/lpips.py on
csrc/lpips.hip) against the SAME module's torch layers in fp32 on the same GPU (``LPIPS.torch_pairs``: nn.Conv2d through the
vendor library, with the value-range check's host read that torchmetrics pays as well), at the two image sizes
scripts/bench_image_eval.py uses.  Both memory formats on both sides: the image as an NCHW-contiguous tensor and as the
[1, 3, H, W] view of an [H, W, 3] image (what get_image_metrics_and_images passes: channels_last in memory; the torch leg
then runs with channels_last weights).  Seeded He-scaled weights (tests/lpips_refs.py; trained ones are not available here),
uniform-noise image and a perturbed copy.  The four legs alternate in one process, `--reps` repetitions after `--warmup`,
each timed with device events around the call; the device clocks are sampled under load.  Appends ONE JSON line per size to
profiles/bench_lpips.jsonl.  Fails without a GPU.
    python scripts/bench_lpips.py [--reps 20] [--warmup 3] [--sizes 1080x1920,900x1600] [--out profiles/bench_lpips.jsonl]"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lpips_refs as R  # noqa: E402
from bench import device_state  # noqa: E402
from neurad_studio_amd.model_components.lpips import LPIPS  # noqa: E402

FP16_MATRIX_PEAK_TFLOPS = 2500.0  # MI355X, dense fp16 MFMA (spec)


def conv_macs(h, w):
    """(real multiply-adds of the five convolutions for ONE image, the same with the image layer's padded reduction: 528
    instead of 363 products per output)"""
    real = issued = 0
    for pool, cin, cout, ks, stride, pad, _ in R.LAYERS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = R.out_size(h, ks, stride, pad), R.out_size(w, ks, stride, pad)
        real += h * w * cout * ks * ks * cin
        issued += h * w * cout * (528 if cin == 3 else ks * ks * cin)
    return real, issued


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    v = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), v


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1080x1920,900x1600")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_lpips.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: no GPU")
    clocks = device_state(0)
    weights = R.make_weights(0)
    m = LPIPS()
    m.load_state_dict(weights)
    m = m.cuda()
    m_cl = copy.deepcopy(m).to(memory_format=torch.channels_last)
    for size in args.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(7)
        img = torch.rand((h, w, 3), generator=g)
        rgb = (img + 0.08 * (torch.rand((h, w, 3), generator=g) - 0.5)).clamp(0, 1)
        img, rgb = img.cuda(), rgb.cuda()
        view = lambda t: torch.moveaxis(t, -1, 0)[None]  # noqa: E731  (models/neurad.py:581-582)
        a_v, b_v = view(img), view(rgb)
        a_c, b_c = a_v.contiguous(), b_v.contiguous()
        legs = {"hip_nchw": lambda: m(a_c, b_c), "hip_hwc_view": lambda: m(a_v, b_v),
                "torch_fp32_nchw": lambda: m.torch_pairs(a_c, b_c).mean(),
                "torch_fp32_channels_last": lambda: m_cl.torch_pairs(a_v, b_v).mean()}
        times, last = {k: [] for k in legs}, {}
        for rep in range(args.warmup + args.reps):
            for k, fn in legs.items():  # alternating in the same process
                ms, v = timed(fn)
                if rep >= args.warmup:
                    times[k].append(ms)
                last[k] = float(v)
        med = {k: median(v) for k, v in times.items()}
        base = min(("torch_fp32_nchw", "torch_fp32_channels_last"), key=med.get)
        hip = min(("hip_nchw", "hip_hwc_view"), key=med.get)
        real, issued = conv_macs(h, w)
        line = {"bench": "lpips", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps,
                "warmup": args.warmup, "height": h, "width": w, "median_ms": med,
                "min_max_ms": {k: [min(v), max(v)] for k, v in times.items()},
                "baseline": base, "ratio_baseline_over_hip": med[base] / med[hip],
                "ratio_same_format": {"nchw": med["torch_fp32_nchw"] / med["hip_nchw"],
                                      "hwc_view": med["torch_fp32_channels_last"] / med["hip_hwc_view"]},
                "conv_gflop_per_call": 2.0 * 2 * real / 1e9, "conv_gflop_issued_per_call": 2.0 * 2 * issued / 1e9,
                "hip_conv_tflops": 2.0 * 2 * real / (med[hip] * 1e-3) / 1e12,
                "hip_fraction_of_fp16_matrix_peak": 2.0 * 2 * real / (med[hip] * 1e-3) / 1e12 / FP16_MATRIX_PEAK_TFLOPS,
                "value": last,
                "note": "one call = LPIPS.forward on one image pair, device events around it, allocations included, no host "
                        "read on the hip legs (the torch legs pay the range check's read, as torchmetrics does); tflops = "
                        "the convolutions' real multiply-adds of both images over the WHOLE call's time, not a kernel's "
                        "share of the peak; seeded weights; one box; not measured here: per-kernel times (profiles/lpips_kernel_stats.txt has "
                        "one trace), the metric inside an ns-eval run, trained weights"}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line))


if __name__ == "__main__":
    main()
