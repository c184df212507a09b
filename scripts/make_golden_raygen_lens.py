"""Golden vectors for device ray generation with a lens (csrc/raygen.hip: nrhip_camera_rays_lens) from the reference's own
generator, in the manner of oracle/make_golden_raygen.py.  Run where the reference tree is present:
    python scripts/make_golden_raygen_lens.py  -> tests/golden/raygen_lens.npz

Six 3848 x 2168 cameras shaped like the ZOD dataparser's (zod_dataparser.py:242-254: FISHEYE, distortion_params =
[k1..k4, 0, 0]) with the poses, times and rolling-shutter metadata of tests/golden/raygen.npz, 512 rays at pixel centres.
Camera 0 has no distortion, cameras 1-3 are radial only, cameras 4-5 have tangential terms as well.  Cases, each from
Cameras.generate_rays (nerfstudio/cameras/cameras.py:332-968):

  fisheye        FISHEYE with the coefficients;
  fisheye_rs     the same with rolling-shutter metadata;
  fisheye_plain  FISHEYE with distortion_params=None;
  persp_dist     PERSPECTIVE with the same coefficients;
  centre         FISHEYE, principal point exactly at a pixel centre (cx = 1924.5, cy = 1084.5): a ray at it and the ray one
                 pixel to its left.  theta = 0 makes the first NaN in direction, norm and pixel area and the second NaN in
                 pixel area (cameras.py:809-814: 0 * 0 / 0); <case>_nan_<quantity> records which elements.

Every case is stored twice: the reference's fp32 result (<case>_<quantity>) and its result with every float camera
tensor and the coords in float64 (<case>_<quantity>_f64), the yardstick of tests/test_gpu_raygen_lens.py.  In that run
the reference's own `.float()` (cameras.py:796-815) still rounds the camera-frame directions to fp32; everything before
and after it is float64.  Everything outside `centre` is asserted finite."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402

ref_import.install()
import synth  # noqa: E402
from nerfstudio.cameras.cameras import Cameras, CameraType  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "raygen_lens.npz")
C, R, W, H = 6, 512, 3848, 2168
QUANTITIES = ("origins", "directions", "pixel_area", "times", "directions_norm")


def inputs():
    """the arrays the fixture stores beside the results (tests build their cameras from these)"""
    base = dict(np.load(os.path.join(ROOT, "tests", "golden", "raygen.npz")))
    dist = np.zeros((C, 6), np.float32)
    # Seeds 39 / 40: draws at which the reference's ten Newton iterations converge for every ray and neighbour.  At
    # these magnitudes many draws leave some ray unconverged (a distortion that folds back inside the image); its fp32
    # and float64 solves then end 1e-4 apart, and bounds taken from such a fixture would say nothing.
    dist[1:, :4] = synth.normal((C - 1, 4), 39) * np.array([0.1, 0.03, 0.01, 0.003], np.float32)
    dist[4:, 4:] = synth.normal((2, 2), 40) * np.float32(0.002)
    coords = np.stack([np.floor(synth.uniform((R,), 0, H, 28)) + 0.5, np.floor(synth.uniform((R,), 0, W, 29)) + 0.5], -1)
    return dict(c2w=base["c2w"], cam_times=base["cam_times"], rolling_shutter_time=base["rolling_shutter_time"],
                time_to_center_pixel=base["time_to_center_pixel"], cam_velocities=base["cam_velocities"],
                fx=synth.uniform((C, 1), 1900, 2100, 23), fy=synth.uniform((C, 1), 1900, 2100, 24),
                cx=synth.uniform((C, 1), 1900, 1950, 25), cy=synth.uniform((C, 1), 1050, 1110, 26), distortion=dist,
                cam_idx=synth.uniform((R,), 0, C, 27).astype(np.int64).clip(0, C - 1), coords=coords.astype(np.float32),
                centre_cx=np.full((C, 1), 1924.5, np.float32), centre_cy=np.full((C, 1), 1084.5, np.float32),
                centre_cam_idx=np.array([1, 1], np.int64), centre_coords=np.array([[1084.5, 1924.5], [1084.5, 1923.5]], np.float32))


def run(g, dtype, camera_type, distortion, rolling_shutter=False, centre=False):
    T = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    md = {"sensor_idxs": torch.arange(C)[:, None]}
    if rolling_shutter:
        md.update(rolling_shutter_time=T(g["rolling_shutter_time"]), time_to_center_pixel=T(g["time_to_center_pixel"]),
                  velocities=T(g["cam_velocities"]))
    pre = "centre_" if centre else ""
    cams = Cameras(camera_to_worlds=T(g["c2w"]), fx=T(g["fx"]), fy=T(g["fy"]), cx=T(g[pre + "cx"]), cy=T(g[pre + "cy"]),
                   width=W, height=H, distortion_params=T(g["distortion"]) if distortion else None, camera_type=camera_type,
                   times=T(g["cam_times"]), metadata=md)
    rb = cams.generate_rays(camera_indices=torch.from_numpy(g[pre + "cam_idx"])[:, None], coords=T(g[pre + "coords"]))
    out = dict(origins=rb.origins, directions=rb.directions, pixel_area=rb.pixel_area, times=rb.times,
               directions_norm=rb.metadata["directions_norm"])
    return {k: v.numpy() for k, v in out.items()}


CASES = {"fisheye": dict(camera_type=CameraType.FISHEYE, distortion=True),
         "fisheye_rs": dict(camera_type=CameraType.FISHEYE, distortion=True, rolling_shutter=True),
         "fisheye_plain": dict(camera_type=CameraType.FISHEYE, distortion=False),
         "persp_dist": dict(camera_type=CameraType.PERSPECTIVE, distortion=True),
         "centre": dict(camera_type=CameraType.FISHEYE, distortion=True, centre=True)}


def generate():
    """-> every array of the fixture"""
    gold = inputs()
    for case, kw in CASES.items():
        for suffix, dtype in (("", torch.float32), ("_f64", torch.float64)):
            for q, v in run(gold, dtype, **kw).items():
                assert v.dtype == (np.float32 if dtype == torch.float32 else np.float64), (case, q, v.dtype)
                assert case == "centre" or np.isfinite(v).all(), f"{case}{suffix}: {q} is not finite"
                gold[f"{case}_{q}{suffix}"] = v
        if case == "centre":
            for q in QUANTITIES:
                gold[f"centre_nan_{q}"] = np.isnan(gold[f"centre_{q}"])
                assert (gold[f"centre_nan_{q}"] == np.isnan(gold[f"centre_{q}_f64"])).all(), q
    return gold


if __name__ == "__main__":
    torch.set_num_threads(1)
    gold = generate()
    np.savez_compressed(OUT, **gold)
    print(OUT, {k: v.shape for k, v in gold.items()})
    for case in CASES:
        for q in QUANTITIES:
            a, b = gold[f"{case}_{q}"].astype(np.float64), gold[f"{case}_{q}_f64"]
            ok = np.isfinite(b)
            print(f"{case:14s} {q:16s} fp32 vs f64: max abs {np.abs(a - b)[ok].max(initial=0.0):.3e}  rel-L2 "
                  f"{np.linalg.norm((a - b)[ok]) / max(np.linalg.norm(b[ok]), 1e-30):.3e}  NaN {int((~ok).sum())}")
