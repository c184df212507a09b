"""Golden vectors for the two per-sample loss terms on packed samples (csrc/losses.hip: nrhip_packed_distortion_loss,
nrhip_packed_lidar_carving) from the reference's own functions on the CPU.  Run where the reference tree is present:
    python scripts/make_golden_packed_losses.py  -> tests/golden/packed_losses.npz

Stored (the inputs come from tests/packed_loss_refs.py and are stored in full next to the results):
  dist_*     nerfstudio_distortion_loss (model_components/losses.py:159-200) on the ragged rays of
             packed_loss_refs.GOLD_COUNTS -- gapped, contiguous, tied-midpoint and zero-width rays -- padded to the longest
             with zero-weight samples and evaluated in float64: loss per ray and its autograd gradient w.r.t. the weights;
  dist_contiguous_loss   lossfun_distortion (losses.py:137-148) on the contiguous rays among them (dist_contiguous_rays);
  carve_*    NeuRADModel._compute_is_close_to_lidar (models/neurad.py:677-700), called as a plain function on a stand-in
             `self` that carries config.loss, over PACKED [M,1] RaySamples whose metadata is gathered per sample, in fp32:
             camera rays, returned and non-returned lidar rays, samples exactly on both boundaries; carve_mask_all_returned
             is the same call without the did_return key."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402

ref_import.install()
import packed_loss_refs as P  # noqa: E402
from nerfstudio.cameras.rays import Frustums, RaySamples  # noqa: E402
from nerfstudio.model_components.losses import lossfun_distortion, nerfstudio_distortion_loss  # noqa: E402
from nerfstudio.models.neurad import NeuRADModel  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "packed_losses.npz")


def distortion(s, e, w, seg):
    """the reference on the rays padded to [R, max_n] with zero-weight samples, float64 -> loss [R], grad [M]"""
    R, n = len(seg) - 1, np.diff(seg)
    S = int(n.max())
    pad = lambda a, fill: np.stack([np.concatenate([a[seg[r]:seg[r + 1]].astype(np.float64),  # noqa: E731
                                                    np.full(S - n[r], fill)]) for r in range(R)])
    starts, ends = torch.from_numpy(pad(s, 0.0))[..., None], torch.from_numpy(pad(e, 0.0))[..., None]
    weights = torch.from_numpy(pad(w, 0.0))[..., None].requires_grad_(True)
    fr = Frustums(origins=torch.zeros(R, S, 3), directions=torch.ones(R, S, 3), starts=starts, ends=ends,
                  pixel_area=torch.ones(R, S, 1))
    rs = RaySamples(frustums=fr, spacing_starts=starts, spacing_ends=ends)
    loss = nerfstudio_distortion_loss(rs, weights=weights)
    assert loss.shape == (R, 1) and loss.dtype == torch.float64
    (g,) = torch.autograd.grad(loss.sum(), weights)
    grad = np.concatenate([g[r, :n[r], 0].numpy() for r in range(R)])
    return loss[:, 0].detach().numpy(), grad


def contiguous(s, e, w, seg):
    """lossfun_distortion on the contiguous rays, one at a time (their lengths differ) -> ray numbers, losses"""
    rays = [r for r in range(len(seg) - 1) if P.kind_of(r) == "contiguous" and seg[r + 1] > seg[r]]
    out = []
    for r in rays:
        b, c = int(seg[r]), int(seg[r + 1])
        assert np.array_equal(e[b:c - 1], s[b + 1:c])
        t = torch.from_numpy(np.concatenate([s[b:c], e[c - 1:c]]).astype(np.float64))[None]
        out.append(float(lossfun_distortion(t, torch.from_numpy(w[b:c].astype(np.float64))[None])[0]))
    return np.array(rays, np.int64), np.array(out)


def is_close(c, with_did_return=True):
    """the reference's mask over packed [M,1] RaySamples with per-sample metadata -> bool [M]"""
    rep = np.diff(c["seg"])
    per = lambda a: torch.from_numpy(np.repeat(a, rep))[:, None, None]  # noqa: E731  ([M,1] samples: [M,1,1] fields)
    M = int(rep.sum())
    fr = Frustums(origins=torch.zeros(M, 1, 3), directions=torch.ones(M, 1, 3), starts=torch.from_numpy(c["t_starts"])[:, None, None],
                  ends=torch.from_numpy(c["t_ends"])[:, None, None], pixel_area=torch.ones(M, 1, 1))
    meta = {"is_lidar": per(c["is_lidar"]), "directions_norm": per(c["distance"])}
    if with_did_return:
        meta["did_return"] = per(c["did_return"])
    rs = RaySamples(frustums=fr, metadata=meta)
    stand_in = types.SimpleNamespace(config=types.SimpleNamespace(loss=types.SimpleNamespace(
        carving_epsilon=P.EPS, non_return_lidar_distance=P.NON_RETURN)))
    NeuRADModel._compute_is_close_to_lidar(stand_in, rs)
    mask = rs.metadata["is_close_to_lidar"]
    assert rs.shape == (M, 1) and mask.shape == (M, 1, 1) and mask.dtype == torch.bool
    return mask[:, 0, 0].numpy()


def generate():
    s, e, w, seg = P.distortion_case(P.GOLD_COUNTS)
    loss, grad = distortion(s, e, w, seg)
    rays, closs = contiguous(s, e, w, seg)
    c = P.carving_case()
    gold = {"dist_s": s, "dist_e": e, "dist_w": w, "dist_seg": seg, "dist_loss": loss, "dist_grad": grad,
            "dist_contiguous_rays": rays, "dist_contiguous_loss": closs,
            "carve_eps": np.float32(P.EPS), "carve_non_return": np.float32(P.NON_RETURN),
            "carve_mask": is_close(c), "carve_mask_all_returned": is_close(c, with_did_return=False)}
    gold.update({f"carve_{k}": v for k, v in c.items()})
    return gold


if __name__ == "__main__":
    torch.set_num_threads(1)
    gold = generate()
    np.savez_compressed(OUT, **gold)
    print(OUT, os.path.getsize(OUT), "bytes")
    s, e, w, seg = (gold[f"dist_{k}"] for k in ("s", "e", "w", "seg"))
    ql, qg = P.distortion_quadratic(s, e, w, seg)
    n, X, S = P.distortion_scales(s, e, w, seg)
    print("distortion: O(n^2) restatement vs reference, worst error / float64 term:",
          float(np.max(np.abs(ql - gold["dist_loss"]) / np.maximum(P.float64_term(n, X, S, 2), 1e-300))), "(loss)",
          float(np.max(np.abs(qg - gold["dist_grad"]) / np.maximum(np.repeat(P.float64_term(n, X, S, 1), np.diff(seg)), 1e-300))),
          "(grad)")
    c = P.carving_case()
    mine = P.carving_mask(c["t_starts"], c["t_ends"], c["seg"], c["is_lidar"], c["did_return"], c["distance"])
    print("carving: restatement == reference:", np.array_equal(mine, gold["carve_mask"]), " close samples:",
          int(gold["carve_mask"].sum()), "of", len(mine), " boundary samples (ray 13: 20..23, ray 14: 30, 31):",
          gold["carve_mask"][c["seg"][13] + 20:c["seg"][13] + 24], gold["carve_mask"][c["seg"][14] + 30:c["seg"][14] + 32])
