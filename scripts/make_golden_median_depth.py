"""Golden vectors for the median depth (csrc/median_depth.hip: nrhip_median_depth) from the reference's own
DepthRenderer(method="median") (model_components/renderers.py:353-397) on the CPU, where torch.cumsum accumulates fp32 in
float64 -- the numerics the contract in include/neurad_hip.h fixes for both devices.  Run where the reference tree is
present:
    python scripts/make_golden_median_depth.py  -> tests/golden/median_depth.npz

Stored: for every S of median_depth_refs.SHAPES the reference's depth [R,1] of median_depth_refs.dense_case(S) (the inputs
are regenerated from their seeds by the tests and checked against `w_sum_<S>`, `s_sum_<S>`, `e_sum_<S>`: float64 sums that
pin them), and the constructed rays with their inputs in full.  The NaN rays are not here: the reference's answer for them
is an artefact of its binary search."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402

ref_import.install()
import median_depth_refs as M  # noqa: E402
from nerfstudio.cameras.rays import Frustums, RaySamples  # noqa: E402
from nerfstudio.model_components.renderers import DepthRenderer  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "median_depth.npz")


def reference(w, starts, ends):
    """the reference's renderer on [R,S] arrays -> depth [R,1]"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))[..., None]  # noqa: E731
    R = w.shape[0]
    fr = Frustums(origins=torch.zeros(R, 1, 3), directions=torch.ones(R, 1, 3), starts=T(starts), ends=T(ends),
                  pixel_area=torch.ones(R, 1, 1))
    depth = DepthRenderer(method="median")(weights=T(w), ray_samples=RaySamples(frustums=fr))
    assert depth.shape == (R, 1) and depth.dtype == torch.float32
    return depth.numpy()


def generate():
    gold = {"shapes": np.array(M.SHAPES, np.int64), "n_rays": np.int64(M.R)}
    for S in M.SHAPES:
        w, s, e = M.dense_case(S)
        gold[f"depth_{S}"] = reference(w, s, e)
        for tag, a in (("w", w), ("s", s), ("e", e)):
            gold[f"{tag}_sum_{S}"] = M.checksum(a)
    w, s, e, index = M.constructed_case()
    gold.update(constructed_w=w, constructed_starts=s, constructed_ends=e, constructed_index=index,
                constructed_depth=reference(w, s, e))
    return gold


if __name__ == "__main__":
    torch.set_num_threads(1)
    gold = generate()
    np.savez_compressed(OUT, **gold)
    print(OUT, os.path.getsize(OUT), "bytes")
    for S in M.SHAPES:
        w, s, e = M.dense_case(S)
        depth, index = M.median_depth(w, s, e)
        never = int((np.cumsum(w.astype(np.float64), -1)[:, -1] < 0.5).sum())
        print(f"S {S:4d}: restatement == reference: {np.array_equal(depth, gold[f'depth_{S}'])}  distinct crossings "
              f"{len(np.unique(index))}  rays that never reach 0.5: {never}")
    w, s, e, index = M.constructed_case()
    depth, idx = M.median_depth(w, s, e)
    print("constructed: depth equal", np.array_equal(depth, gold["constructed_depth"]), "index", idx[:, 0], "expected", index)
