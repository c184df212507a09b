"""The VGG perceptual loss at the flagship batch -- 40 rendered + 40 target patches of 96 x 96 -- forward + backward:
model_components/perceptual.py (one autograd node on csrc/vgg_loss.hip) against the restated torch network
(tests/vgg_refs.py: the reference's construction; the reference tree is not on the GPU machine) under
torch.autocast(float16), which is what a user of the reference's module runs through MIOpen.  The torch network is run twice,
with NCHW-contiguous and with channels_last tensors and weights; the faster of the two is the baseline.  Seeded He-scaled
weights (torchvision's are not available here), uniform images.  Every leg backpropagates loss * 65536 (GradScaler's initial
scale, as the reference's trainer does) and the values are compared with one untimed fp32 run of the torch network.
The three legs alternate in one process, `--reps` repetitions after `--warmup`, each timed with device events around forward
+ backward; the device clocks are sampled under load.  Appends ONE JSON line to profiles/bench_vgg_loss.jsonl.  Fails
without a GPU.
    python scripts/bench_vgg_loss.py [--reps 20] [--warmup 5] [--patches 40] [--size 96] [--out profiles/bench_vgg_loss.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vgg_refs as R  # noqa: E402
from bench import device_state  # noqa: E402
from neurad_studio_amd.model_components.perceptual import VGGPerceptualLoss  # noqa: E402


def conv_macs(size):
    """multiply-adds of the 13 convolutions for ONE image"""
    h = w = size
    total = 0
    for st in R.steps():
        if st[0] == "conv":
            total += h * w * 9 * st[3] * st[4]
        elif st[0] == "pool":
            h, w = h // 2, w // 2
    return total


def torch_leg(net, x, y, channels_last):
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    with torch.autocast("cuda", dtype=torch.float16):
        z = torch.cat([x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)], dim=0).contiguous(memory_format=fmt)
        loss = 0
        for w, f in zip(net.weights, net.vgg(z)):
            fx, fy = f.chunk(2, dim=0)
            loss = loss + w * torch.nn.functional.l1_loss(fx, fy.detach())
    return loss


LOSS_SCALE = 65536.0  # torch.amp.GradScaler's initial scale, which the reference's trainer backpropagates under autocast:
#                       without it the fp16 gradients of the torch legs underflow (tap 1 starts at 1.3e-9)


def timed(fn, x):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = fn()
    (g,) = torch.autograd.grad(loss * LOSS_SCALE, x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), loss.detach(), g / LOSS_SCALE


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--patches", type=int, default=40)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_vgg_loss.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vgg_loss: no GPU")
    clocks = device_state(0)
    weights = R.make_weights(0)
    hip = VGGPerceptualLoss()
    hip.load_state_dict(weights)
    hip = hip.cuda()
    nets = {}
    for name, cl in (("torch_nchw", False), ("torch_channels_last", True)):
        net = R.ReferenceStyleLoss()
        net.load_state_dict(weights)
        net = net.cuda()
        nets[name] = (net.to(memory_format=torch.channels_last) if cl else net, cl)
    x, y = R.make_images(args.patches, args.size, args.size, seed=3)
    x, y = x.cuda().requires_grad_(True), y.cuda()
    legs = {"hip": lambda: hip(x, y)}
    for name, (net, cl) in nets.items():
        legs[name] = (lambda net=net, cl=cl: torch_leg(net, x, y, cl))
    times = {k: [] for k in legs}
    last = {}
    for rep in range(args.warmup + args.reps):
        for k, fn in legs.items():  # alternating in the same process
            ms, loss, g = timed(fn, x)
            if rep >= args.warmup:
                times[k].append(ms)
            last[k] = (float(loss), g)
    base = min(("torch_nchw", "torch_channels_last"), key=lambda k: median(times[k]))
    macs = conv_macs(args.size) * (2 * args.patches + args.patches)  # forward on both halves, input gradients on one
    # not timed: the same network in fp32 (no autocast), the yardstick the three fp16 legs' values are compared with
    _, loss32, g32 = timed(lambda: nets["torch_nchw"][0](x, y), x)
    last["torch_fp32_untimed"] = (float(loss32), g32)
    gref = g32.double()
    line = {"bench": "vgg_perceptual_loss", "device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps,
            "warmup": args.warmup, "patches": args.patches, "size": args.size,
            "median_ms": {k: median(v) for k, v in times.items()},
            "min_max_ms": {k: [min(v), max(v)] for k, v in times.items()},
            "baseline": base, "ratio_baseline_over_hip": median(times[base]) / median(times["hip"]),
            "conv_tflop_per_step": 2.0 * macs / 1e12,
            "hip_conv_tflops": 2.0 * macs / (median(times["hip"]) * 1e-3) / 1e12,
            "loss": {k: v[0] for k, v in last.items()},
            "grad_rel_l2_vs_fp32": {k: float((v[1].double() - gref).norm() / gref.norm()) for k, v in last.items()},
            "note": "one call = forward + backward to the rendered images, device events around it, allocations included; "
                    "the tflops figure is the convolutions' multiply-adds over the whole call's time, not a kernel's share "
                    "of the fp16 matrix peak; gradients are taken of loss * 65536 and divided again (GradScaler's "
                    "initial scale); the fp16 legs' gradients differ from the fp32 network's by percents because ReLU masks "
                    "and L1 signs flip with every rounding (tests/test_gpu_vgg_loss.py)"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
