"""Lidar scan evaluation: the float64 restatement of the nearest-neighbour / chamfer op and of the lidar branch of
``NeuRADModel.get_image_metrics_and_images`` (models/neurad.py:589-620), the synthetic scan both the fixture generator
(scripts/make_golden_lidar_eval.py) and the tests use, and the error bounds.  numpy float64, direct differences; used by
tests/test_lidar_eval_host.py, tests/test_gpu_lidar_eval.py and tests/test_gpu_lidar_eval_model.py.

Why a restatement and not the reference's function: ``chamfer_distance`` (utils/math.py:745-798) accumulates into
``torch.tensor(0.0)`` (fp32 whatever the inputs are) and takes its distances from ``torch.cdist``'s |a|^2 + |b|^2 - 2ab form.

Per-element bound (``U6``).  The kernel computes, in fp32 with every operation rounded once (the library builds with
-ffp-contract=off; the two ``fmaf`` it writes only REMOVE roundings),

    dx = fl(qx - tx), dy = fl(qy - ty), dz = fl(qz - tz)          |d. - exact| <= u |exact|,  u = 2^-24
    sx = fl(dx dx), sy = fl(dy dy), sz = fl(dz dz)                each (1 + u)^2 (1 + u) of its exact square
    d  = fl(fl(sx + sy) + sz)                                     two more factors (1 + u) on sx and sy, one on sz

All three terms are non-negative, so the relative error of the sum is at most that of its worst term:
(1 + u)^5 - 1 for the x and y terms (two from the squared difference, one square, two adds), which is < 6 u.  The same holds
for each candidate j, and a minimum of values each within 6 u of its exact value lies within 6 u of the exact minimum.
Hence |got_i - ref_i| <= 6 u ref_i, with ref_i the exact (float64) value on the fp32-rounded inputs.

Sum bound (``U8``): every term within 6 u; the float64 accumulation of at most a few thousand non-negative terms adds
n 2^-53 << u; the final rounding to fp32 adds u; one more u of margin: |got - ref| <= 8 u ref.
"""
import numpy as np

import synth

U = 2.0 ** -24
U6 = 6 * U
U8 = 8 * U
CASES = ("ray_drop", "distance", "fallback")  # ray_drop_loss_mult > 0; == 0; nothing predicted to return
NON_RETURN_DISTANCE = 150.0  # LossSettings.non_return_lidar_distance of the reference (models/neurad.py)
METRIC_KEYS = ("depth_median_l2", "depth_mean_rel_l2", "intensity_rmse", "ray_drop_accuracy", "chamfer_distance")


def nearest_sq_dist(query, target, query_valid=None, target_valid=None, rows=512):
    """float64 [N]: min over the valid targets of |q - t|^2 by direct differences; +inf without a valid target (or for a
    query with a NaN coordinate), 0 for an invalid query; a target with a NaN coordinate never wins"""
    q = np.asarray(query, np.float64)[:, :3]
    t = np.asarray(target, np.float64)[:, :3]
    if target_valid is not None:
        t = t[np.asarray(target_valid).astype(bool).reshape(-1)]
    out = np.full((q.shape[0],), np.inf)
    if t.shape[0]:
        for i in range(0, q.shape[0], rows):
            d = ((q[i:i + rows, None, :] - t[None, :, :]) ** 2).sum(-1)
            out[i:i + rows] = np.where(np.isnan(d), np.inf, d).min(axis=1)
    if query_valid is not None:
        out = np.where(np.asarray(query_valid).astype(bool).reshape(-1), out, 0.0)
    return out


def chamfer(source, target, source_valid=None, target_valid=None, normalize_with_target=False):
    """float64 scalar: sum over the valid sources + sum over the valid targets of the nearest squared distances, divided by
    the number of valid targets when ``normalize_with_target`` (IEEE: +inf / NaN for empty sets)"""
    n, m = len(source), len(target)
    sv = np.ones(n, bool) if source_valid is None else np.asarray(source_valid).astype(bool).reshape(-1)
    tv = np.ones(m, bool) if target_valid is None else np.asarray(target_valid).astype(bool).reshape(-1)
    s2t = nearest_sq_dist(source, target, sv, tv)[sv].sum()
    t2s = nearest_sq_dist(target, source, tv, sv)[tv].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        return (s2t + t2s) / (np.float64(tv.sum()) if normalize_with_target else np.float64(1.0))


def lidar_metrics(depth, intensity, ray_drop_logits, pred_points, scan, distance, did_return, ray_drop_loss_mult,
                  non_return_distance=NON_RETURN_DISTANCE):
    """the lidar branch of get_image_metrics_and_images (models/neurad.py:596-620) in float64 on the given (fp32) arrays:
    depth / intensity / ray_drop_logits / distance [n,1], pred_points [n, >= 3], scan [n, >= 4], did_return [n] bool.
    The predicted-return decisions are taken on the fp32 values, as the model takes them."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    ret = np.asarray(did_return).astype(bool).reshape(-1)
    d, gt = f(depth).reshape(-1), f(distance).reshape(-1)
    sq = (d - gt)[ret] ** 2
    out = {"depth_median_l2": np.sort(sq)[(len(sq) - 1) // 2],  # torch.median: the lower middle value
           "depth_mean_rel_l2": (((d - gt) / gt)[ret] ** 2).mean(),
           "intensity_rmse": np.sqrt(((f(intensity).reshape(-1) - f(scan)[:, 3])[ret] ** 2).mean())}
    logits32 = np.asarray(ray_drop_logits, np.float32).reshape(-1)
    prob32 = (1.0 / (1.0 + np.exp(-logits32.astype(np.float64)))).astype(np.float32)
    out["ray_drop_accuracy"] = np.float64(np.mean((prob32 > 0.5) == ~ret))
    if ray_drop_loss_mult > 0.0:
        pred_ret = prob32 < 0.5
    else:
        pred_ret = np.asarray(depth, np.float32).reshape(-1) < np.float32(non_return_distance)
    if pred_ret.any() and ret.any():
        out["chamfer_distance"] = chamfer(pred_points, scan, pred_ret, ret, normalize_with_target=True)
    else:
        out["chamfer_distance"] = np.linalg.norm(f(scan)[ret, :3], axis=-1).mean()
    return out


def scan(n=3000, seed=600):
    """a synthetic scan and a model's predictions for it: points [n,5] (xyz inside +-80 x +-80 x +-4 m in the lidar frame,
    intensity, time offset), a quarter of the beams without a return, and for every ray a predicted depth, intensity,
    ray-drop logit and predicted point (the true point displaced by a few decimetres).  Logits stay away from 0 and depths
    away from the non-return distance, so that no decision hangs on the last bit of a sigmoid."""
    xyz = np.stack([synth.uniform((n,), -80, 80, seed), synth.uniform((n,), -80, 80, seed + 1),
                    synth.uniform((n,), -4, 4, seed + 2)], -1)
    pts = np.concatenate([xyz, synth.uniform((n, 1), 0, 1, seed + 3), synth.uniform((n, 1), -0.05, 0.05, seed + 4)], -1)
    did_return = synth.uniform((n,), 0, 1, seed + 5) < 0.75
    distance = np.linalg.norm(xyz, axis=-1, keepdims=True).astype(np.float32)
    depth = (distance * (1.0 + 0.02 * synth.normal((n, 1), seed + 6))).astype(np.float32)
    far = synth.uniform((n,), 0, 1, seed + 7) < 0.2  # predicted not to return by distance
    depth[far] = np.float32(400.0) + synth.uniform((int(far.sum()), 1), 0, 50, seed + 8)
    sign = np.where(synth.uniform((n, 1), 0, 1, seed + 9) < 0.7, -1.0, 1.0)  # 70 % predicted to return by probability
    logits = (sign * synth.uniform((n, 1), 0.3, 3.0, seed + 10)).astype(np.float32)
    pred_points = (xyz + 0.3 * synth.normal((n, 3), seed + 11)).astype(np.float32)
    return dict(points=pts.astype(np.float32), did_return=did_return, distance=distance, depth=depth,
                intensity=synth.uniform((n, 1), 0, 1, seed + 12), ray_drop_logits=logits, pred_points=pred_points)


def case_inputs(g, case):
    """(depth, ray_drop_logits, ray_drop_loss_mult) of one fixture case: ``fallback`` predicts no return for any ray"""
    if case == "ray_drop":
        return g["depth"], g["ray_drop_logits"], 0.01
    if case == "distance":
        return g["depth"], g["ray_drop_logits"], 0.0
    return g["depth"], np.abs(g["ray_drop_logits"]), 0.01
