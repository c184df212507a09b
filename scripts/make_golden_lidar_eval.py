"""Golden vectors for the evaluation of a lidar scan (csrc/lidar_eval.hip, integration/neurad_hip.py: fused_lidar_eval) from
the reference's own code, in the manner of scripts/make_golden_raygen_lens.py.  Run where the reference tree is present:
    python scripts/make_golden_lidar_eval.py  -> tests/golden/lidar_eval.npz

The scan and the predictions are tests/lidar_eval_refs.py:scan (3000 beams inside +-80 x +-80 x +-4 m, a quarter without a
return).  For each case of lidar_eval_refs.CASES -- ray_drop (ray_drop_loss_mult > 0: returns predicted by probability),
distance (ray_drop_loss_mult == 0: by depth < non_return_lidar_distance), fallback (no ray predicted to return) -- stored:

  ref_<case>_<metric>      the lidar branch of the reference's NeuRADModel.get_image_metrics_and_images
                           (models/neurad.py:589-620), fp32 on the CPU, called on a real reference model
  f64_<case>_<metric>      the float64 restatement (lidar_eval_refs.lidar_metrics) on the same fp32 arrays
  ref_<case>_chamfer       the reference's chamfer_distance(pred, target, 1_000, True) (utils/math.py:745-798) on the case's
                           point sets (fallback: every predicted point against the returned ones), fp32
  f64_<case>_chamfer       the restatement's value on the same sets
  gap_<case>               |ref - f64| / f64 of the two chamfer values: what separates the reference's fp32 chunked
                           |a|^2 + |b|^2 - 2ab sums from exact arithmetic on the same inputs (tests allow 4 x this)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402

ref_import.install()
import lidar_eval_refs as R  # noqa: E402
import plugin_harness as t  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lidar_eval.npz")


def reference_model():
    import nerfstudio.models.neurad as ref_neurad
    from nerfstudio.data.scene_box import SceneBox

    ref_neurad.VGGPerceptualLossPix2Pix = torch.nn.Identity  # (torchvision's weights are absent; not used here)
    cfg = t.shrink(ref_neurad.NeuRADModelConfig(implementation="torch"))
    return cfg.setup(scene_box=SceneBox(aabb=torch.tensor([[-100.0] * 3, [100.0] * 3])), num_train_data=2,
                     metadata={"duration": 5.0, "sensor_idx_to_name": {0: "cam0", 1: "cam1", 2: "lidar"}, "trajectories": []})


def generate():
    from nerfstudio.utils.math import chamfer_distance

    g = R.scan()
    gold = dict(g)
    model = reference_model().eval()
    T = torch.from_numpy
    for case in R.CASES:
        depth, logits, mult = R.case_inputs(g, case)
        model.config.loss.ray_drop_loss_mult = mult
        outputs = {"depth": T(depth), "intensity": T(g["intensity"]), "ray_drop_logits": T(logits), "points": T(g["pred_points"])}
        batch = {"lidar": T(g["points"]), "distance": T(g["distance"]), "did_return": T(g["did_return"])[:, None],
                 "is_lidar": torch.ones(len(depth), 1, dtype=torch.bool)}
        with torch.no_grad():
            metrics, _ = model.get_image_metrics_and_images(outputs, batch)
        want = R.lidar_metrics(depth, g["intensity"], logits, g["pred_points"], g["points"], g["distance"], g["did_return"], mult)
        assert set(metrics) == set(R.METRIC_KEYS) == set(want), (set(metrics), set(want))
        for k in R.METRIC_KEYS:
            gold[f"ref_{case}_{k}"] = np.float32(float(metrics[k]))
            gold[f"f64_{case}_{k}"] = np.float64(want[k])
        # the chamfer call alone, on the case's point sets
        prob = T(logits).sigmoid().squeeze(-1)
        pred_ret = (prob < 0.5) if mult > 0 else (T(depth) < model.config.loss.non_return_lidar_distance).squeeze(-1)
        if not pred_ret.any():
            pred_ret = torch.ones_like(pred_ret)
        src, tgt = T(g["pred_points"])[pred_ret], T(g["points"])[T(g["did_return"]), :3]
        ref_cd = float(chamfer_distance(src, tgt, 1_000, True))
        f64_cd = float(R.chamfer(src.numpy(), tgt.numpy(), normalize_with_target=True))
        gold[f"ref_{case}_chamfer"], gold[f"f64_{case}_chamfer"] = np.float32(ref_cd), np.float64(f64_cd)
        gold[f"gap_{case}"] = np.float64(abs(ref_cd - f64_cd) / f64_cd)
    return gold


if __name__ == "__main__":
    torch.set_num_threads(1)
    gold = generate()
    np.savez_compressed(OUT, **gold)
    print(OUT, os.path.getsize(OUT), "bytes")
    for case in R.CASES:
        print(case, "gap", gold[f"gap_{case}"], {k: (float(gold[f"ref_{case}_{k}"]), float(gold[f"f64_{case}_{k}"]))
                                                 for k in R.METRIC_KEYS})
