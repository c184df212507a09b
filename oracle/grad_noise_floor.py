"""Reference-vs-reference noise floor of the composed training step's gradients, per loss term of get_loss_dict and per kind
of parameter, on the batches of tests/test_gpu_reference_plugin.py (build container or GPU box, CPU only).  Two yardsticks:

  fp32_vs_fp64   the reference's own torch model in fp32 against the same model in fp64;
  perturbed_max  the reference in fp32 against itself with its inputs moved at the fp32 ROUNDING LEVEL -- hash-table
                 entries and ray origins multiplied by (1 + 1.2e-7 n), n ~ N(0, 1): what any other correct fp32
                 implementation of the forward differs by -- elementwise max over PERTURBED_TRIALS draws.

For each (term, kind): rel-L2, the fraction of units (table rows / elements) further than 1e-4 of the tensor's largest unit
from the reference, and the rel-L2 over the remaining units (tests/test_gpu_reference_plugin.py:_outlier_stats).

What the floor is made of: the LOSS VALUES of two runs agree to 1e-7, the gradients of the lidar terms only to ~1e-3 -- a
handful of the hidden units of mlp_geo sit within 5e-5 of the ReLU kink (the fp32 positions of far samples move the
level-8192 features by that much), flip between the two runs, and each flip switches one sample's whole contribution on or
off: few units far off (outlier_frac), the others close (rest_rel_l2 1e-5 .. 6e-4: flips of low-gradient samples stay under
the 1e-4 outlier threshold).  The plugin-vs-reference test on the GPU
holds the HIP path to the same picture (check_gradients_against_floor) instead of to a widened rel-L2.
Scenes: static, actors3, both with camera_optimizer.mode = "SO3xR3" (*_pose: also the floor of the ray gradients), and
actors32 (config[4] at test size: 32 actors, tables holding fp16-representable values).
TEST INFRASTRUCTURE.   python oracle/grad_noise_floor.py  ->  profiles/r05_grad_noise_floor.json"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
import numpy as np
import torch

import plugin_harness as t

PERTURBED_TRIALS = int(os.environ.get("NRHIP_FLOOR_TRIALS", "8"))
t.ref_import.install()
os.environ["NERFSTUDIO_METHOD_CONFIGS"] = "neurad-hip=neurad_studio_amd.integration.neurad_hip:neurad_hip"
import nerfstudio.models.neurad as ref_neurad

ref_neurad.VGGPerceptualLossPix2Pix = torch.nn.Identity
torch.nn.Module.to = lambda self, *a, **k: self  # (build_pair moves the plugin to cuda: not here)


def step(m, b, dt, origin_noise=None):
    m.zero_grad(set_to_none=True)
    rb = t.bundle(b, "cpu")
    lab = t.labels(b, "cpu")
    if origin_noise is not None:
        rb.origins = rb.origins * origin_noise
    if dt == torch.float64:
        for k in ("origins", "directions", "pixel_area", "times"):
            setattr(rb, k, getattr(rb, k).double())
        rb.metadata["directions_norm"] = rb.metadata["directions_norm"].double()
        lab = {k: (v.double() if v.is_floating_point() else v) for k, v in lab.items()}
    o = m.get_outputs(rb, patch_size=(b["patch"], b["patch"]), calc_lidar_losses=True)
    met = m.get_metrics_dict(o, lab)
    return rb, m.get_loss_dict(o, lab, met)


def ray_grads(rb, losses):
    return torch.autograd.grad(sum(losses.values()), [rb.origins, rb.directions], retain_graph=True)


def merge_max(acc, new):
    for term, kinds in new.items():
        for kind, st in kinds.items():
            cur = acc.setdefault(term, {}).setdefault(kind, dict(st))
            for k, v in st.items():
                cur[k] = max(cur[k], v)
    return acc


def main():
    out = {}
    for wa, pose, na in ((False, False, 3), (False, True, 3), (True, False, 3), (True, True, 3), (True, False, 32)):
        scene = ("actors%d" % na if wa else "static") + ("_pose" if pose else "")
        if os.environ.get("NRHIP_FLOOR_SCENES") and scene not in os.environ["NRHIP_FLOOR_SCENES"].split(","):
            continue
        if True:
            kw = dict(pose_opt=pose, n_actors=na, fp16_tables=na == 32)  # (actors32: tables hold fp16-representable values)
            _, m32 = t.build_pair(ref_neurad, wa, **kw)
            _, m64 = t.build_pair(ref_neurad, wa, **kw)
            m64 = m64.double()
            b = t.batch(wa, n_actors=na)
            t.deterministic(m32, True), t.deterministic(m64, True)
            rb32, l32 = step(m32, b, torch.float32)
            rb64, l64 = step(m64, b, torch.float64)
            f64 = t.per_loss_gradient_errors(m32, l32, m64, l64, detail=True)
            if pose:
                f64["__ray_grads__"] = [t.rel_l2(t.N(a), t.N(c)) for a, c in zip(ray_grads(rb32, l32), ray_grads(rb64, l64))]
            pert = {}
            for trial in range(PERTURBED_TRIALS):
                _, mp = t.build_pair(ref_neurad, wa, **kw)
                t.deterministic(mp, True)
                g = torch.Generator().manual_seed(1000 + trial)
                with torch.no_grad():
                    for n, p in mp.named_parameters():
                        if n.endswith("hash_table"):
                            p.mul_(1 + 1.2e-7 * torch.randn(p.shape, generator=g))
                noise = 1 + 1.2e-7 * torch.randn((len(b["o"]), 3), generator=g)
                _, lp = step(mp, b, torch.float32, origin_noise=noise)
                merge_max(pert, t.per_loss_gradient_errors(mp, lp, m32, l32, detail=True))
            out[scene] = {"fp32_vs_fp64": f64, "perturbed_max": pert, "perturbed_trials": PERTURBED_TRIALS}
            print(scene, json.dumps({k: ({a: (float(f"{s['rel_l2']:.1e}"), s["n_outliers"], float(f"{s['rest_rel_l2']:.1e}"))
                                          for a, s in v.items()} if isinstance(v, dict) else v) for k, v in f64.items()}))
            print(scene, "perturbed_max", json.dumps({k: {a: (float(f"{s['rel_l2']:.1e}"), s["n_outliers"],
                                                             float(f"{s['rest_rel_l2']:.1e}")) for a, s in v.items()}
                                                      for k, v in pert.items()}), flush=True)
    path = os.path.join(ROOT, "profiles", "r05_grad_noise_floor.json")
    if os.environ.get("NRHIP_FLOOR_SCENES") and os.path.exists(path):  # a partial run updates its scenes only
        out = dict(json.load(open(path)), **out)
    json.dump(out, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
