"""Fused field kernels on the grids with L * F < 32 against the operator-level path of the same field.

For each (L, F) it times, at 4096 rays x 128 samples and at BASELINE config[0]'s 512 x 32 (32-wide MLPs, SDF head):
  * eval:  NeuRADField.render (one fused kernel)  vs  Field.forward on the operator kernels + weights + compositing;
  * train: Field.forward + backward through FieldTrainFn  vs  the same with fused_training = False.
A and B alternate in one process after a warm-up; device events; medians.  One JSON line per shape and size.
    python scripts/bench_field_shapes.py [--reps 20] [--warmup 5]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neurad_studio_amd import ops  # noqa: E402
from neurad_studio_amd.cameras.rays import RayBundle  # noqa: E402
from neurad_studio_amd.field_components.field_heads import FieldHeadNames as FH  # noqa: E402
from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig  # noqa: E402
from neurad_studio_amd.model_components.ray_samplers import PowerSampler  # noqa: E402

SHAPES = [(1, 4), (4, 2), (4, 4), (8, 2)]
SIZES = [(4096, 128), (512, 32)]


def make_field(L, F, lg=18):
    cfg = NeuRADFieldConfig()
    st = cfg.grid.static
    st.num_levels, st.hashgrid_dim, st.log2_hashmap_size = L, F, lg
    if L == 1:
        st.base_res = st.max_res = 32
    fld = NeuRADField(cfg, actors=None, static_scale=100.0).cuda()
    with torch.no_grad():
        fld.hashgrid.static_grid.hash_table.mul_(1000.0)  # O(1) features: alphas vary
    return fld


def rays(R, S, gen):
    o = torch.randn(R, 3, generator=gen) * torch.tensor([5.0, 5.0, 0.5])
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    rb = RayBundle(origins=o.cuda(), directions=d.cuda(), pixel_area=torch.full((R, 1), 2.7e-7, device="cuda"),
                   nears=torch.zeros(R, 1, device="cuda"), fars=torch.full((R, 1), 200.0, device="cuda"))
    return rb, PowerSampler(num_samples=S, lambda_=-1.0, scaling=0.1).eval()(rb)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    for L, F in SHAPES:
        fld = make_field(L, F)
        for R, S in SIZES:
            rb, rs = rays(R, S, gen)
            o, d, area = rb.origins, rb.directions, rb.pixel_area[:, 0]
            starts, ends = rs.frustums.starts[..., 0].contiguous(), rs.frustums.ends[..., 0].contiguous()

            def eval_fused():
                with torch.no_grad():
                    fld.render(o, d, area, starts, ends)

            def eval_op():
                with torch.no_grad():
                    fld.fused_supported = lambda with_actors=False: False  # Field.forward takes the operator kernels
                    out = fld(rs)
                    del fld.fused_supported
                    w, _ = ops.render_weight_from_alpha(out[FH.ALPHA][..., 0].contiguous())
                    ops.composite_fwd(w, out[FH.FEATURE].contiguous(), starts, ends)

            def train(fused):
                def step():
                    fld.fused_training = fused
                    out = fld(rs)
                    (out[FH.FEATURE].square().mean() + out[FH.ALPHA].mean()).backward()
                    fld.zero_grad(set_to_none=True)
                return step

            res = {}
            for name, a_fn, b_fn in (("eval", eval_fused, eval_op), ("train", train(True), train(False))):
                for _ in range(args.warmup):
                    a_fn(), b_fn()
                ta, tb = [], []
                for _ in range(args.reps):  # A and B alternate
                    ta.append(timed(a_fn))
                    tb.append(timed(b_fn))
                res[name] = (median(ta), median(tb))
            fld.fused_training = True
            print(json.dumps({"L": L, "F": F, "H": 32, "rays": R, "samples": S,
                              "eval_fused_us": round(res["eval"][0], 1), "eval_operator_us": round(res["eval"][1], 1),
                              "eval_speedup": round(res["eval"][1] / res["eval"][0], 2),
                              "train_fused_us": round(res["train"][0], 1), "train_operator_us": round(res["train"][1], 1),
                              "train_speedup": round(res["train"][1] / res["train"][0], 2),
                              "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
