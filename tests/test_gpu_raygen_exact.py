"""The perspective and lidar ray kernels (csrc/raygen.hip) against their numpy float32 restatement (tests/raygen_refs.py,
pinned to the reference by tests/test_raygen_refs_host.py), bit for bit and element by element.

Both kernels use only + - * / sqrt and fmaf, all correctly rounded on the device (the build keeps the IEEE divide and sqrt,
fp32 denormals are on), so the expected relation is equality of the bits, not a tolerance.  A NaN equals a NaN of any sign
and payload (raygen_refs.same_bits).  Every call goes through the C ABI into outputs that are pre-filled with a sentinel
and 64 rows longer than the launch: the rows below R must all have been written, the rows past R must not."""
import numpy as np
import pytest
import torch

import raygen_refs as rr
from gpu_util import cuda

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A5A5A5A  # as float32 1.5e16: no output of any case
PERSPECTIVE = 1  # CameraType value
OUT_WIDTHS = dict(origins=3, directions=3, pixel_area=1, directions_norm=1, times=1)


def outputs(R, lidar=False):
    out = {q: torch.full((R + GUARD, w), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
           for q, w in OUT_WIDTHS.items()}
    if lidar:
        out["did_return"] = torch.full((R + GUARD, 1), SENTINEL & 0xFF, dtype=torch.uint8, device="cuda")
    return out


def untouched(t):
    """per row: every element still holds the sentinel"""
    a = t.cpu().numpy()
    return ((a.view(np.uint32) == SENTINEL) if a.dtype == np.float32 else (a == SENTINEL & 0xFF)).all(-1)


def tables(tab, names):
    """arrays of a case -> device tensors (kept by the caller) ; None stays None"""
    return {k: None if tab.get(k) is None else cuda(np.ascontiguousarray(tab[k], dtype=np.float32)) for k in names}


def run_camera(tab, cam_idx, coords, mode, entry="nrhip_camera_rays", distortion=None, times_out=True):
    """-> the five outputs with their guard rows, as device tensors"""
    from neurad_studio_amd import _lib
    from neurad_studio_amd.ops import launch

    R = cam_idx.shape[0]
    d = tables(tab, ("c2w", "fx", "fy", "cx", "cy", "times", "rolling_shutter_time", "time_to_center_pixel", "velocities",
                     "extent"))
    t = _lib.CameraTable()
    (t.camera_to_worlds, t.fx, t.fy, t.cx, t.cy, t.times, t.rolling_shutter_time, t.time_to_center_pixel, t.velocities,
     t.shutter_extent) = (0 if v is None else v.data_ptr() for v in d.values())
    t.rolling_shutter = mode
    out = outputs(R)
    args = [cuda(cam_idx), cuda(coords), R, out["origins"], out["directions"], out["pixel_area"], out["directions_norm"],
            out["times"] if times_out else None]
    if entry == "nrhip_camera_rays":
        launch(entry, t, *args)
    else:
        lens = _lib.CameraLens()
        lens.camera_type = PERSPECTIVE
        table = None if distortion is None else cuda(distortion)
        lens.distortion = 0 if table is None else table.data_ptr()
        launch(entry, t, lens, *args)
    torch.cuda.synchronize()
    return out


def run_lidar(tab, lidar_idx, points, ego, threshold=rr.THRESHOLD):
    from neurad_studio_amd import _lib
    from neurad_studio_amd.ops import launch

    R = lidar_idx.shape[0]
    d = tables(tab, ("l2w", "times", "velocities", "hdiv", "vdiv"))
    t = _lib.LidarTable()
    t.lidar_to_worlds, t.times, t.velocities, t.horizontal_beam_divergence, t.vertical_beam_divergence = (
        0 if v is None else v.data_ptr() for v in d.values())
    t.assume_ego_compensated, t.valid_lidar_distance_threshold = int(ego), threshold
    out = outputs(R, lidar=True)
    launch("nrhip_lidar_rays", t, cuda(lidar_idx), cuda(points), points.shape[1], R, out["origins"], out["directions"],
           out["pixel_area"], out["directions_norm"], out["did_return"], out["times"])
    torch.cuda.synchronize()
    return out


def assert_exact(out, want, R, what):
    """every element of every output below R has the restatement's bits; below R nothing holds the sentinel, past R
    everything does"""
    for q, t in out.items():
        got = t.cpu().numpy()
        assert got.shape[0] == R + GUARD
        assert untouched(t)[R:].all(), f"{what}: {q} written past row {R}"
        assert not untouched(t)[:R].any(), f"{what}: {q} has rows below {R} that were not written"
        same = rr.same_bits(got[:R], want[q])
        if not same.all():
            rows = np.nonzero(~same.all(-1))[0]
            r = rows[0]
            u = rr.ulps(got[:R], want[q]).max() if got.dtype == np.float32 else -1
            raise AssertionError(f"{what}: {q} differs on {rows.size} of {R} rays (up to {u} ulp), first ray {r}: kernel "
                                 f"{got[r]} restatement {want[q][r]}")


def differing_rays(a, b):
    return int((~rr.same_bits(a, b)).any(-1).sum())


# ---- launch geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 255, 256, 257, 1000])
def test_launch_geometry(R):
    """one thread; a last block one short of full, full, and one over; four blocks with a ragged last one"""
    tab, idx, coords = rr.camera_case(R)
    want = rr.camera_rays(tab, idx, coords, 1)
    assert_exact(run_camera(tab, idx, coords, 1), want, R, f"camera_rays R={R}")
    zeros = np.zeros((tab["fx"].shape[0], 6), np.float32)
    assert_exact(run_camera(tab, idx, coords, 1, "nrhip_camera_rays_lens", zeros), want, R, f"camera_rays_lens R={R}")
    tab, idx, pts = rr.lidar_case(R, 5)
    assert_exact(run_lidar(tab, idx, pts, False), rr.lidar_rays(tab, idx, pts, False), R, f"lidar_rays R={R}")


def test_no_rays_no_launch():
    for run, case in ((lambda *a: run_camera(*a, 1), rr.camera_case(4)),
                      (lambda *a: run_camera(*a, 1, "nrhip_camera_rays_lens"), rr.camera_case(4)),
                      (lambda *a: run_lidar(*a, True), rr.lidar_case(4, 5))):
        tab, idx, rows = case
        out = run(tab, idx[:0], rows[:0])
        assert all(t.shape[0] == GUARD and untouched(t).all() for t in out.values())


# ---- cameras -----------------------------------------------------------------------------------------------------------
R_CAMERA = 777  # four blocks, the last one ragged; ~130 rays per camera


@pytest.fixture(scope="module")
def camera():
    return rr.camera_case(R_CAMERA)


@pytest.fixture(scope="module")
def camera_refs(camera):
    """rolling-shutter mode -> restatement; mode 0 without a times table"""
    tab, idx, coords = camera
    return {mode: rr.camera_rays(rr.without(tab, "times") if mode == 0 else tab, idx, coords, mode) for mode in range(4)}


def test_the_camera_case_holds_what_it_is_meant_to(camera, camera_refs):
    tab, idx, coords = camera
    assert set(idx.tolist()) == set(range(6)), "the camera varies from ray to ray"
    y, x = coords[:, 0], coords[:, 1]
    on_pp = (x == tab["cx"][idx]) & (y == tab["cy"][idx])
    assert on_pp.sum() > 50 and (coords < 0).any() and (coords == 1e6).any() and (coords % 1 == 0.5).any()
    want = camera_refs[1]
    ok = ~np.isin(idx, (rr.CAM_ZERO, rr.CAM_NAN))
    near = ok & ~(coords == 1e6).any(-1)  # at 1e6 a pixel's step is below the resolution of a unit vector's components
    assert np.isfinite(want["directions"][ok]).all() and (want["pixel_area"][near] > 0).all()
    n = want["directions_norm"][:, 0]
    assert n[idx == rr.CAM_SMALL].max() < 1 and n[idx == rr.CAM_LARGE].min() > 999
    zero = idx == rr.CAM_ZERO  # a zero rotation block: the clamp, a zero direction, no pixel area
    assert (n[zero] == rr.EPS).all() and (want["directions"][zero] == 0).all() and (want["pixel_area"][zero] == 0).all()
    nan = idx == rr.CAM_NAN
    assert nan.sum() > 50 and np.isnan(n[nan]).all() and np.isnan(want["directions"][nan]).all()
    assert np.isnan(want["pixel_area"][nan]).all() and np.isfinite(want["origins"]).all() and np.isfinite(want["times"]).all()
    # the two roundings of the norm differ on many of these rays: a kernel with the other one cannot pass
    old = rr.camera_rays(tab, idx, coords, 1, fused=False)
    assert differing_rays(old["directions"], want["directions"]) > 20
    assert differing_rays(old["directions_norm"], want["directions_norm"]) > 20
    assert differing_rays(old["pixel_area"], want["pixel_area"]) > 60  # three norms meet in a pixel area


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_camera_rays_exact(camera, camera_refs, mode):
    tab, idx, coords = camera
    if mode == 0:
        tab = rr.without(tab, "times", "rolling_shutter_time", "time_to_center_pixel", "velocities", "extent")
    assert_exact(run_camera(tab, idx, coords, mode), camera_refs[mode], R_CAMERA, f"camera_rays mode {mode}")


def test_camera_rays_without_rolling_shutter_copy_the_times_table(camera):
    tab, idx, coords = camera
    want = rr.camera_rays(tab, idx, coords, 0)
    assert (want["times"][:, 0] == tab["times"][idx]).all() and (want["origins"] == tab["c2w"][idx][:, :, 3]).all()
    assert_exact(run_camera(tab, idx, coords, 0), want, R_CAMERA, "camera_rays mode 0 with times")
    # no times output: the other four are written all the same, and that one is left alone
    out = run_camera(rr.without(tab, "times"), idx, coords, 0, times_out=False)
    assert untouched(out.pop("times")).all()
    del want["times"]
    assert_exact(out, want, R_CAMERA, "camera_rays mode 0, times NULL")


@pytest.mark.parametrize("table", ["null", "zeros"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_lens_entry_point_without_distortion_exact(camera, camera_refs, mode, table):
    """nrhip_camera_rays_lens, PERSPECTIVE: it shares finish_camera_ray, and an all-zero table skips the solve"""
    tab, idx, coords = camera
    if mode == 0:
        tab = rr.without(tab, "times")
    distortion = None if table == "null" else np.zeros((6, 6), np.float32)
    out = run_camera(tab, idx, coords, mode, "nrhip_camera_rays_lens", distortion)
    assert_exact(out, camera_refs[mode], R_CAMERA, f"camera_rays_lens mode {mode}, distortion {table}")


def test_a_nan_pose_stays_with_its_camera(camera):
    tab, idx, coords = camera
    clean_tab, clean_idx, clean_coords = rr.camera_case(R_CAMERA, nan_pose=False)
    assert np.array_equal(idx, clean_idx) and np.array_equal(coords, clean_coords)
    with_nan, clean = run_camera(tab, idx, coords, 2), run_camera(clean_tab, idx, coords, 2)
    others = idx != rr.CAM_NAN
    for q in OUT_WIDTHS:
        a, b = with_nan[q].cpu().numpy()[:R_CAMERA], clean[q].cpu().numpy()[:R_CAMERA]
        assert np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32)), q
        if q in ("directions", "pixel_area", "directions_norm"):
            assert np.isnan(a[~others]).all() and np.isfinite(b[~others]).all(), q
        else:
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), q
    assert_exact(clean, rr.camera_rays(clean_tab, idx, coords, 2), R_CAMERA, "camera_rays, finite pose")


# ---- lidars ------------------------------------------------------------------------------------------------------------
R_LIDAR = 600  # three blocks, the last one ragged


@pytest.mark.parametrize("ego", [True, False])
@pytest.mark.parametrize("point_dim", [3, 4, 5, 6])
def test_lidar_rays_exact(point_dim, ego):
    tab, idx, pts = rr.lidar_case(R_LIDAR, point_dim)
    want = rr.lidar_rays(tab, idx, pts, ego)
    assert_exact(run_lidar(tab, idx, pts, ego), want, R_LIDAR, f"lidar_rays point_dim {point_dim} ego {ego}")
    if point_dim < 5:  # no time offset: the sensor does not move, the scan's time is the ray's
        assert (want["origins"] == tab["l2w"][idx][:, :, 3]).all() and (want["times"][:, 0] == tab["times"][idx]).all()
    else:
        assert (want["origins"] != tab["l2w"][idx][:, :, 3]).any(-1).sum() > R_LIDAR // 2
    if point_dim == 6:  # column 5 is not read
        five = rr.lidar_rays(tab, idx, np.ascontiguousarray(pts[:, :5]), ego)
        assert all(rr.same_bits(five[q], want[q]).all() for q in five)


@pytest.mark.parametrize("ego", [True, False])
def test_lidar_rays_without_velocities_or_times(ego):
    tab, idx, pts = rr.lidar_case(R_LIDAR, 5)
    moving = rr.lidar_rays(tab, idx, pts, ego)
    still = rr.lidar_rays(rr.without(tab, "velocities"), idx, pts, ego)
    assert_exact(run_lidar(rr.without(tab, "velocities"), idx, pts, ego), still, R_LIDAR, "lidar_rays, velocities NULL")
    # only the times move: origins are the translations, the time offset still counts
    assert (still["origins"] == tab["l2w"][idx][:, :, 3]).all() and rr.same_bits(still["times"], moving["times"]).all()
    assert (still["times"][:, 0] != tab["times"][idx]).sum() > R_LIDAR // 2
    no_times = rr.lidar_rays(rr.without(tab, "times"), idx, pts, ego)
    assert (no_times["times"][:, 0] == pts[:, 4]).all()
    assert_exact(run_lidar(rr.without(tab, "times"), idx, pts, ego), no_times, R_LIDAR, "lidar_rays, times NULL")
    neither = rr.without(tab, "times", "velocities")
    assert_exact(run_lidar(neither, idx, pts, ego), rr.lidar_rays(neither, idx, pts, ego), R_LIDAR, "lidar_rays, both NULL")


@pytest.mark.parametrize("ego", [True, False])
@pytest.mark.parametrize("point_dim", [3, 5])
def test_lidar_edges(point_dim, ego):
    """a point at the sensor, the two sides of the valid-distance threshold, a NaN coordinate"""
    tab, idx, pts = rr.lidar_case(R_LIDAR, point_dim)
    out = run_lidar(tab, idx, pts, ego)
    assert_exact(out, rr.lidar_rays(tab, idx, pts, ego), R_LIDAR, f"lidar_rays point_dim {point_dim} ego {ego}")
    got = {q: t.cpu().numpy()[:R_LIDAR] for q, t in out.items()}
    dist, ret = got["directions_norm"][:, 0], got["did_return"][:, 0]
    assert dist[rr.ROW_ORIGIN] == rr.EPS and ret[rr.ROW_ORIGIN] == 1 and (got["directions"][rr.ROW_ORIGIN] == 0).all()
    assert dist[rr.ROW_AT_THRESHOLD] == 1000.0 and ret[rr.ROW_AT_THRESHOLD] == 0  # strictly less
    assert dist[rr.ROW_BELOW_THRESHOLD] == np.nextafter(np.float32(1000), np.float32(0)) and ret[rr.ROW_BELOW_THRESHOLD] == 1
    assert np.isnan(dist[rr.ROW_NAN]) and ret[rr.ROW_NAN] == 0 and np.isnan(got["directions"][rr.ROW_NAN]).all()
    assert np.isfinite(got["origins"]).all() and np.isfinite(got["times"]).all() and 0 < ret.sum() < R_LIDAR - 10
    # the NaN stays in its row
    clean_tab, clean_idx, clean_pts = rr.lidar_case(R_LIDAR, point_dim, nan_point=False)
    clean = run_lidar(clean_tab, clean_idx, clean_pts, ego)
    others = np.arange(R_LIDAR) != rr.ROW_NAN
    for q, t in clean.items():
        b = t.cpu().numpy()[:R_LIDAR]
        assert np.array_equal(got[q][others], b[others]) and np.isfinite(b).all(), q
    assert clean["did_return"][rr.ROW_NAN] == 1
