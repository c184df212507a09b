"""One occupancy-grid update at 128^3, L in {1, 4}, during warm-up (every visible cell is a candidate) and after it
(res^3 / 4 uniform draws + the occupied cells per level).  Timed with device events after a warm-up, alternating in one process:
  (a) OccGridEstimator._update (csrc/occgrid_update.h) with a trivial occ_eval_fn (three elementwise torch ops);
  (b) the same with the proposal field's density_fn (one hash-grid kernel over all candidates);
  (c) what a user had before: the same rule as a torch-op composition on the same GPU (nonzero / boolean indexing / indexed
      assignment per level, a boolean-index mean), with the trivial occ_eval_fn.
Appends ONE JSON line to profiles/bench_occgrid_update.jsonl: medians and their spread (min, max, interquartile range), the
host synchronisations per update of each variant (counted by torch's sync debug mode), the bytes the rule must move computed
from shapes, and (a)'s bytes/s over the 8 TB/s HBM peak as a WHOLE-CALL figure (it contains occ_eval_fn).  No ratio is asked
for: the line says whether (a) is faster than (c) beyond the run-to-run spread.  Fails without a GPU.
    python scripts/bench_occgrid_update.py [--reps 20] [--warmup 5] [--out profiles/bench_occgrid_update.jsonl]"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neurad_studio_amd.fields.neurad_field import NeuRADProposalField, NeuRADProposalFieldConfig  # noqa: E402
from neurad_studio_amd.shims.nerfacc import OccGridEstimator  # noqa: E402

HBM_PEAK = 8e12  # bytes/s
RES, AABB, WARMUP_STEPS, THRE, DECAY = 128, [-4.0, -4.0, -4.0, 4.0, 4.0, 4.0], 256, 1e-2, 0.95


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def spread(v):
    s = sorted(v)
    q = lambda f: s[min(int(f * len(s)), len(s) - 1)]  # noqa: E731
    return {"median": q(0.5), "min": s[0], "max": s[-1], "q25": q(0.25), "q75": q(0.75)}


def trivial(p):
    """a blob of radius ~3 around the origin, scaled like density x step size"""
    return torch.clamp(3.0 - p.abs().amax(-1, keepdim=True), 0.0, 1.0) * 0.05


class TorchEstimator:
    """the update rule as torch ops, the way nerfacc's own Python states it (per level: nonzero / boolean index, indexed
    assignment; then a boolean-index mean).  On duplicate cells the indexed assignment keeps an arbitrary writer."""

    def __init__(self, est: OccGridEstimator):
        self.L, self.res, self.cells = est.levels, RES, RES ** 3
        self.aabbs = est.aabbs.clone()
        self.occs = torch.zeros_like(est.occs)
        self.binaries = torch.zeros_like(est.binaries)

    def update(self, step, occ_fn):
        n, res, dev = self.cells // 4, self.res, self.occs.device
        for l in range(self.L):
            occs_l = self.occs[l * self.cells:(l + 1) * self.cells]
            if step < WARMUP_STEPS:
                idx = torch.nonzero(occs_l >= 0)[:, 0]
            else:
                uni = torch.randint(self.cells, (n,), device=dev)
                uni = uni[occs_l[uni] >= 0]
                occupied = torch.nonzero(self.binaries[l].flatten())[:, 0]
                if occupied.shape[0] > n:
                    occupied = occupied[torch.randint(occupied.shape[0], (n,), device=dev)]
                idx = torch.cat([uni, occupied])
            xyz = torch.stack([idx // (res * res), (idx // res) % res, idx % res], -1).float()
            x = (xyz + torch.rand_like(xyz)) / res
            p = self.aabbs[l, :3] + x * (self.aabbs[l, 3:] - self.aabbs[l, :3])
            occ = occ_fn(p).reshape(-1)
            occs_l[idx] = torch.maximum(occs_l[idx] * DECAY, occ)
        thre = torch.clamp(self.occs[self.occs >= 0].mean(), max=THRE)
        self.binaries = (self.occs > thre).view(self.binaries.shape)


def count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w)


def rule_bytes(L, warmup):
    """what one update must move, from shapes: visibility (occs, 4 B/cell) [+ binaries 1 B/cell, draws 8 + 4 B each],
    per candidate slot id 4 B written and read, jitter 12 B, position 12 B, value 4 B; the EMA's read and write of the touched
    cells (<= 8 B per slot); the mean's read of occs and the binaries' write (4 + 1 B/cell).  occ_eval_fn's own traffic is not
    in it."""
    cells, n = RES ** 3, RES ** 3 // 4
    cap = cells if warmup else 2 * n
    per_level = 4 * cells + (0 if warmup else cells + 12 * n) + cap * (8 + 12 + 12 + 4 + 8) + 5 * cells
    return L * per_level


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_occgrid_update.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occgrid_update: no GPU")
    from bench import device_state

    clocks = device_state(0)
    torch.manual_seed(0)
    fld = NeuRADProposalField(NeuRADProposalFieldConfig(), actors=None, static_scale=8.0).cuda().eval()
    density = lambda p: fld.density_fn(p) * 0.05  # noqa: E731  (density x step size)
    cases = {}
    for L in (1, 4):
        for regime, step in (("warmup", 0), ("after_warmup", 10 * WARMUP_STEPS)):
            ests = {"hip_trivial": OccGridEstimator(AABB, RES, L), "hip_density_fn": OccGridEstimator(AABB, RES, L)}
            tor = TorchEstimator(ests["hip_trivial"])
            fns = {"hip_trivial": lambda s, e=ests["hip_trivial"]: e._update(s, trivial, THRE, DECAY, WARMUP_STEPS),
                   "hip_density_fn": lambda s, e=ests["hip_density_fn"]: e._update(s, density, THRE, DECAY, WARMUP_STEPS),
                   "torch_ops_trivial": lambda s: tor.update(s, trivial)}
            for fn in fns.values():  # every variant's grid has seen the scene before it is timed
                fn(0), fn(16)
            syncs = {k: count_syncs(lambda fn=fn: fn(step)) for k, fn in fns.items()}
            times = {k: [] for k in fns}
            for rep in range(args.warmup + args.reps):
                for k, fn in fns.items():  # alternating in the same process
                    t = timed(lambda: fn(step))
                    if rep >= args.warmup:
                        times[k].append(t)
            sp = {k: spread(v) for k, v in times.items()}
            a, c = sp["hip_trivial"], sp["torch_ops_trivial"]
            nbytes = rule_bytes(L, regime == "warmup")
            cases[f"L{L}_{regime}"] = {
                "us": sp, "host_syncs_per_update": syncs, "rule_bytes": nbytes,
                "occupied_share": {"hip": float(ests["hip_trivial"].binaries.float().mean()),
                                   "torch": float(tor.binaries.float().mean())},
                "hip_trivial_whole_call": {"bytes_per_s": nbytes / (a["median"] * 1e-6),
                                           "share_of_8TBps_hbm_peak": nbytes / (a["median"] * 1e-6) / HBM_PEAK,
                                           "note": "the rule's bytes over the whole call's time, occ_eval_fn included"},
                "ratio_hip_over_torch": a["median"] / c["median"],
                "hip_faster_beyond_spread": a["max"] < c["min"],
            }
    line = {"bench": "occgrid_update", "grid": RES, "aabb": AABB, "device": torch.cuda.get_device_name(0), "clocks": clocks,
            "reps": args.reps, "warmup": args.warmup, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
