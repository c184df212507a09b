"""The cameras of tests/golden/raygen_lens.npz (scripts/make_golden_raygen_lens.py) as the attribute bag
``cameras.raygen.camera_rays`` takes, and the distances the lens tests compare."""
import types

import numpy as np
import torch

from conftest import rel_l2

PERSPECTIVE, FISHEYE, EQUIRECTANGULAR = 1, 2, 3  # CameraType values
W, H = 3848, 2168
# case of the fixture -> (camera type, distortion_params given, rolling shutter, the centre inputs)
CASES = {"fisheye": (FISHEYE, True, False, False), "fisheye_rs": (FISHEYE, True, True, False),
         "fisheye_plain": (FISHEYE, False, False, False), "persp_dist": (PERSPECTIVE, True, False, False),
         "centre": (FISHEYE, True, False, True)}
QUANTITIES = ("origins", "directions", "pixel_area", "times", "directions_norm")


def cameras(g, to, camera_type=FISHEYE, distortion=True, rolling_shutter=False, centre=False):
    """``to``: array -> tensor on the device under test"""
    C = g["c2w"].shape[0]
    md = {"sensor_idxs": to(np.arange(C)[:, None])}
    if rolling_shutter:
        md.update(rolling_shutter_time=to(g["rolling_shutter_time"]), time_to_center_pixel=to(g["time_to_center_pixel"]),
                  velocities=to(g["cam_velocities"]))
    pre = "centre_" if centre else ""
    return types.SimpleNamespace(
        camera_to_worlds=to(g["c2w"]), fx=to(g["fx"]), fy=to(g["fy"]), cx=to(g[pre + "cx"]), cy=to(g[pre + "cy"]),
        width=to(np.full((C, 1), W)), height=to(np.full((C, 1), H)), times=to(g["cam_times"]), metadata=md,
        camera_type=to(np.full((C, 1), camera_type)), distortion_params=to(g["distortion"]) if distortion else None)


def case_inputs(g, case, to):
    """-> (cameras, camera_indices [R,1], coords [R,2]) of a case of the fixture"""
    camera_type, distortion, rolling_shutter, centre = CASES[case]
    pre = "centre_" if centre else ""
    return (cameras(g, to, camera_type, distortion, rolling_shutter, centre), to(g[pre + "cam_idx"])[:, None],
            to(g[pre + "coords"]))


def bundle_arrays(rb):
    """the five quantities of a generated bundle as host arrays"""
    out = dict(origins=rb.origins, directions=rb.directions, pixel_area=rb.pixel_area, times=rb.times,
               directions_norm=rb.metadata["directions_norm"])
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def distance(q, a, b):
    """the norms of tests/test_gpu_raygen.py: max abs for directions, origins and times, rel-L2 for pixel area and norm"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if q in ("pixel_area", "directions_norm"):
        return rel_l2(a, b)
    return float(np.abs(a - b).max(initial=0.0))
