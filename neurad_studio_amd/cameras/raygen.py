"""Ray generation on the device: drop-in for ``Cameras.generate_rays(camera_indices, coords)`` and
``Lidars.generate_rays(lidar_indices, points)`` of the reference (nerfstudio/cameras/cameras.py:560-968,
cameras/lidars.py:399-460), one HIP kernel each (csrc/raygen.hip).

``camera_rays`` covers PERSPECTIVE and FISHEYE cameras (one type per ``Cameras`` object), with the reference's Newton
undistortion of ``distortion_params`` (camera_utils.py:655-758) inside the kernel: FISHEYE with or without coefficients
(the ZOD dataparser's cameras), PERSPECTIVE with non-zero coefficients only on request (``undistort_perspective=True``).
Mixed types and every other camera type (FISHEYE624, equirectangular, VR180 / ODS, orthophoto) raise
NotImplementedError; ``distortion_params_delta`` and ``camera_opt_to_camera`` are not taken.  Mirrored from the
reference: a FISHEYE ray exactly at the principal point is NaN (theta = 0 in u sin(theta) / theta), and the pixel area of
the rays one pixel to its left / above it is NaN.

``cameras`` / ``lidars`` are the reference's own objects (or anything with the same tensor attributes: camera_to_worlds,
fx, fy, cx, cy, width, height, times, metadata, camera_type, distortion_params | lidar_to_worlds, times, metadata,
horizontal_beam_divergence, vertical_beam_divergence, assume_ego_compensated, valid_lidar_distance_threshold).  The
result is a RayBundle of the class passed as ``bundle_cls`` (default: this package's; pass the reference's to stay
inside nerfstudio types)."""
from __future__ import annotations

import weakref
from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from ..ops import _chk, launch
from .rays import RayBundle

PERSPECTIVE, FISHEYE = 1, 2  # CameraType values (cameras/cameras.py:43-55)


def _f32(t: Tensor) -> Tensor:
    return _chk(t.reshape(t.shape[0], -1).to(torch.float32), "sensor table")


_ELIGIBLE: dict = {}  # id(cameras) -> (key, camera type, distorted, error message | None)
# id(cameras) -> the object an entry was made for: a weak reference, or the object itself where its type takes none (it then
# lives as long as its entry).  An id -- and with the caching allocator the tensors' addresses, versions and shapes, i.e. the
# whole key -- comes back once an object is freed: without this a NEW Cameras object could meet a dead one's entry.
_OWNER: dict = {}


def _owns(cameras) -> bool:
    own = _OWNER.get(id(cameras))
    return own is cameras or (isinstance(own, weakref.ref) and own() is cameras)


def _check_cameras(cameras, undistort_perspective: bool):
    """-> (camera type, distorted) of a Cameras object the kernels cover: one type, PERSPECTIVE or FISHEYE.  The unique()
    and any() read the device, i.e. they synchronise the host with the stream: they run ONCE per Cameras object (keyed on the
    identity and in-place version of its two tensors), not once per training step."""
    ct, dp = cameras.camera_type, getattr(cameras, "distortion_params", None)
    key = tuple((t.data_ptr(), t._version, tuple(t.shape)) if isinstance(t, Tensor) else None for t in (ct, dp))
    hit = _ELIGIBLE.get(id(cameras))
    if hit is None or hit[0] != key or not _owns(cameras):
        types = [PERSPECTIVE] if ct is None else torch.unique(ct).tolist()
        err = None
        if len(types) != 1:  # the reference's own loop (cameras.py:792-800) only fills the first matching type's rays
            err = f"device ray generation needs cameras of one type, got types {types}"
        elif types[0] not in (PERSPECTIVE, FISHEYE):
            err = (f"device ray generation covers PERSPECTIVE and FISHEYE cameras, not type {types[0]}; use "
                   "Cameras.generate_rays otherwise")
        distorted = dp is not None and bool((dp != 0).any())
        if len(_ELIGIBLE) >= 64:
            _ELIGIBLE.clear(), _OWNER.clear()
        hit = _ELIGIBLE[id(cameras)] = (key, types[0], distorted, err)
        try:
            _OWNER[id(cameras)] = weakref.ref(cameras)
        except TypeError:
            _OWNER[id(cameras)] = cameras
    _, camera_type, distorted, err = hit
    if err is None and camera_type == PERSPECTIVE and distorted and not undistort_perspective:
        err = ("device ray generation covers undistorted PERSPECTIVE cameras unless undistort_perspective=True; use "
               "Cameras.generate_rays otherwise")
    if err is not None:
        raise NotImplementedError(err)
    return camera_type, distorted


def camera_rays(cameras, camera_indices: Tensor, coords: Tensor, bundle_cls=RayBundle, *, undistort_perspective: bool = False):
    """camera_indices [R,1] (or [R]) long, coords [R,2] = (y, x) pixel-centre coordinates.  FISHEYE cameras, with or without
    ``distortion_params``, are covered as they are; PERSPECTIVE cameras with non-zero ``distortion_params`` only with
    ``undistort_perspective=True``."""
    camera_type, distorted = _check_cameras(cameras, undistort_perspective)
    idx = _chk(camera_indices.reshape(-1).long(), "camera_indices", torch.int64)
    xy = _chk(coords.reshape(-1, 2).to(torch.float32), "coords")
    R, dev = idx.shape[0], idx.device
    keep = [_f32(cameras.camera_to_worlds), _f32(cameras.fx), _f32(cameras.fy), _f32(cameras.cx), _f32(cameras.cy)]
    t = _lib.CameraTable()
    t.camera_to_worlds, t.fx, t.fy, t.cx, t.cy = (k.data_ptr() for k in keep)
    times_tab = None if cameras.times is None else _f32(cameras.times)
    t.times = 0 if times_tab is None else times_tab.data_ptr()
    md = cameras.metadata or {}
    rs = all(k in md for k in ("rolling_shutter_time", "time_to_center_pixel", "velocities"))
    if rs:
        direction = md.get("rs_direction")
        t.rolling_shutter = {"Horizontal": 2, "Horizontal_reversed": 3}.get(direction, 1)
        extent = _f32((cameras.height if t.rolling_shutter == 1 else cameras.width).to(torch.float32))
        keep += [_f32(md["rolling_shutter_time"]), _f32(md["time_to_center_pixel"]), _f32(md["velocities"]), extent]
        t.rolling_shutter_time, t.time_to_center_pixel, t.velocities, t.shutter_extent = (k.data_ptr() for k in keep[-4:])
    o = torch.empty((R, 3), device=dev)
    d = torch.empty((R, 3), device=dev)
    area = torch.empty((R, 1), device=dev)
    norm = torch.empty((R, 1), device=dev)
    times = None if times_tab is None else torch.empty((R, 1), device=dev)
    if camera_type == PERSPECTIVE and not distorted:
        launch("nrhip_camera_rays", t, idx, xy, R, o, d, area, norm, times)
    else:
        lens = _lib.CameraLens()
        lens.camera_type = camera_type
        if distorted:  # all-zero coefficients pass through the solve bit for bit: NULL skips it
            table = _f32(cameras.distortion_params)
            if table.shape != (keep[0].shape[0], 6):
                raise ValueError(f"distortion_params: expected [{keep[0].shape[0]}, 6], got {tuple(table.shape)}")
            lens.distortion = table.data_ptr()
        launch("nrhip_camera_rays_lens", t, lens, idx, xy, R, o, d, area, norm, times)
    skip = ("rolling_shutter_time", "time_to_center_pixel", "rs_direction") if rs else ()
    metadata = {k: v[idx] for k, v in md.items() if isinstance(v, Tensor) and k not in skip}
    metadata["directions_norm"] = norm
    return bundle_cls(origins=o, directions=d, pixel_area=area, camera_indices=idx[:, None], times=times, metadata=metadata,
                      fars=torch.full_like(area, 1_000_000.0))


def lidar_rays(lidars, lidar_indices: Tensor, points: Tensor, bundle_cls=RayBundle):
    """lidar_indices [R,1] (or [R]) long, points [R, >=4]: xyz (lidar frame), intensity, time offset in the sweep."""
    idx = _chk(lidar_indices.reshape(-1).long(), "lidar_indices", torch.int64)
    pts = _chk(points.reshape(idx.shape[0], -1).to(torch.float32), "points")
    R, dev = idx.shape[0], idx.device
    md = lidars.metadata or {}
    keep = [_f32(lidars.lidar_to_worlds), _f32(lidars.horizontal_beam_divergence), _f32(lidars.vertical_beam_divergence)]
    t = _lib.LidarTable()
    t.lidar_to_worlds, t.horizontal_beam_divergence, t.vertical_beam_divergence = (k.data_ptr() for k in keep)
    times_tab = None if lidars.times is None else _f32(lidars.times)
    vel = _f32(md["velocities"]) if "velocities" in md else None
    t.times = 0 if times_tab is None else times_tab.data_ptr()
    t.velocities = 0 if vel is None else vel.data_ptr()
    t.assume_ego_compensated = int(bool(lidars.assume_ego_compensated))
    t.valid_lidar_distance_threshold = float(lidars.valid_lidar_distance_threshold)
    o = torch.empty((R, 3), device=dev)
    d = torch.empty((R, 3), device=dev)
    area = torch.empty((R, 1), device=dev)
    dist = torch.empty((R, 1), device=dev)
    ret = torch.empty((R, 1), device=dev, dtype=torch.uint8)
    times = None if times_tab is None else torch.empty((R, 1), device=dev)
    launch("nrhip_lidar_rays", t, idx, pts, pts.shape[1], R, o, d, area, dist, ret, times)
    metadata = {k: v[idx] for k, v in md.items() if isinstance(v, Tensor)}
    metadata.update(directions_norm=dist, is_lidar=torch.ones((R, 1), dtype=torch.bool, device=dev), did_return=ret.bool())
    return bundle_cls(origins=o, directions=d, pixel_area=area, camera_indices=idx[:, None], times=times, metadata=metadata,
                      fars=torch.full_like(area, 1_000_000.0))
