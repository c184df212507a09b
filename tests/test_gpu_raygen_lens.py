"""Device ray generation for FISHEYE and lens-distorted cameras (csrc/raygen.hip: nrhip_camera_rays_lens) against the
reference's own generator (tests/golden/raygen_lens.npz from Cameras.generate_rays, scripts/make_golden_raygen_lens.py).

The yardstick is the reference run with float64 camera tensors and coords.  For every quantity the kernel may be at most
twice as far from it as the reference's own fp32 run is: the device's sinf / cosf / divide may differ from the CPU's by an
ulp, and in the worst case the kernel's error adds to the reference's.  Both distances come from the fixture and are
printed.  Where the fp32 reference is at distance 0 (origins and times without rolling shutter are copies) so must the
kernel be."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import cuda
from raygen_lens_cases import (CASES, EQUIRECTANGULAR, FISHEYE, PERSPECTIVE, QUANTITIES, bundle_arrays, cameras, case_inputs,
                               distance)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return load_golden("raygen_lens")


def run_case(g, case, rows=None):
    from neurad_studio_amd.cameras.raygen import camera_rays

    cams, idx, coords = case_inputs(g, case, cuda)
    return camera_rays(cams, idx[:rows], coords[:rows], undistort_perspective=case == "persp_dist")


def check_against_fixture(g, case, got, keep=None):
    """keep: per quantity, the elements to compare (default all)"""
    for q in QUANTITIES:
        sel = slice(None) if keep is None else keep[q]
        f64 = g[f"{case}_{q}_f64"][sel]
        ours, theirs = distance(q, got[q][sel], f64), distance(q, g[f"{case}_{q}"][sel], f64)
        print(f"{case} {q}: kernel {ours:.3e}, fp32 reference {theirs:.3e} from the float64 run")
        assert ours <= 2 * theirs, (case, q, ours, theirs)


@pytest.mark.parametrize("case", ["fisheye", "fisheye_rs", "fisheye_plain", "persp_dist"])
def test_camera_rays_vs_reference(g, case):
    rb = run_case(g, case)
    got = bundle_arrays(rb)
    assert all(np.isfinite(v).all() for v in got.values())
    check_against_fixture(g, case, got)
    # the bundle of the undistorted path: keys, shapes, metadata
    assert torch.equal(rb.metadata["sensor_idxs"][:, 0], cuda(g["cam_idx"])) and "rolling_shutter_time" not in rb.metadata
    assert float(rb.fars.min()) == 1_000_000.0 and rb.camera_indices.shape == (512, 1)
    assert rb.origins.shape == rb.directions.shape == (512, 3) and rb.pixel_area.shape == rb.times.shape == (512, 1)


def test_principal_point_is_nan_where_the_reference_is(g):
    """theta = 0: the reference's u sin(theta) / theta is 0 * 0 / 0.  Mirrored, not repaired."""
    got = bundle_arrays(run_case(g, "centre"))
    for q in QUANTITIES:
        np.testing.assert_array_equal(np.isnan(got[q]), g[f"centre_nan_{q}"], err_msg=q)
        assert np.isfinite(got[q][~g[f"centre_nan_{q}"]]).all(), q
    assert g["centre_nan_directions"][0].all() and g["centre_nan_pixel_area"].all() and not g["centre_nan_directions"][1].any()
    check_against_fixture(g, "centre", got, keep={q: ~g[f"centre_nan_{q}"] for q in QUANTITIES})


def equal_bundles(a, b, rows=slice(None)):
    a, b = bundle_arrays(a), bundle_arrays(b)
    return all(np.array_equal(a[q][rows].view(np.uint32), b[q][rows].view(np.uint32)) for q in QUANTITIES)


def test_zero_coefficients_give_the_bits_of_no_distortion(g):
    from neurad_studio_amd.cameras.raygen import camera_rays

    plain = run_case(g, "fisheye_plain")
    cams, idx, coords = case_inputs(g, "fisheye", cuda)
    # camera 0 of the fixture has an all-zero row in a table that is not all zero: the kernel's own pass-through
    rows = g["cam_idx"] == 0
    assert rows.any() and not g["distortion"][0].any() and g["distortion"][1:].any()
    assert equal_bundles(camera_rays(cams, idx, coords), plain, rows)
    cams.distortion_params = torch.zeros_like(cams.distortion_params)
    assert equal_bundles(camera_rays(cams, idx, coords), plain)


def test_perspective_without_distortion_gives_the_bits_of_camera_rays():
    """nrhip_camera_rays_lens, PERSPECTIVE, distortion NULL against nrhip_camera_rays on the inputs of raygen.npz, rolling
    shutter included"""
    from neurad_studio_amd import _lib
    from neurad_studio_amd.ops import launch

    b = load_golden("raygen")
    C, R = b["c2w"].shape[0], b["cam_idx"].shape[0]
    tabs = [cuda(b[k].reshape(C, -1)) for k in ("c2w", "fx", "fy", "cx", "cy", "cam_times", "rolling_shutter_time",
                                                 "time_to_center_pixel", "cam_velocities")]
    tabs.append(torch.full((C, 1), 1080.0, device="cuda"))
    t = _lib.CameraTable()
    (t.camera_to_worlds, t.fx, t.fy, t.cx, t.cy, t.times, t.rolling_shutter_time, t.time_to_center_pixel, t.velocities,
     t.shutter_extent) = (k.data_ptr() for k in tabs)
    idx, coords = cuda(b["cam_idx"]), cuda(b["coords"])
    for mode in (0, 1):
        t.rolling_shutter = mode
        outs = [[torch.full((R, n), -7.0, device="cuda") for n in (3, 3, 1, 1, 1)] for _ in range(2)]
        lens = _lib.CameraLens()
        lens.camera_type = PERSPECTIVE
        launch("nrhip_camera_rays", t, idx, coords, R, *outs[0])
        launch("nrhip_camera_rays_lens", t, lens, idx, coords, R, *outs[1])
        for old, new in zip(*outs):
            assert torch.equal(old.view(torch.int32), new.view(torch.int32)) and bool((old != -7.0).any()), mode


def test_results_do_not_depend_on_the_launch_geometry(g):
    full = run_case(g, "fisheye")
    assert equal_bundles(run_case(g, "fisheye"), full)  # two runs of the same call
    for n in (1, 257):  # one thread of one block; a second block with one ray
        part = bundle_arrays(run_case(g, "fisheye", rows=n))
        whole = bundle_arrays(full)
        for q in QUANTITIES:
            assert part[q].shape[0] == n and np.array_equal(part[q].view(np.uint32), whole[q][:n].view(np.uint32)), (n, q)


def test_the_gate(g):
    from neurad_studio_amd.cameras import raygen

    idx, coords = cuda(g["cam_idx"])[:, None], cuda(g["coords"])
    cams = cameras(g, cuda, FISHEYE)
    raygen.camera_rays(cams, idx, coords)  # FISHEYE is accepted
    entry = raygen._ELIGIBLE[id(cams)]
    assert entry[1:] == (FISHEYE, True, None)
    raygen.camera_rays(cams, idx, coords)
    assert raygen._ELIGIBLE[id(cams)] is entry  # the second call found it: no device read
    mixed = cameras(g, cuda, FISHEYE)
    mixed.camera_type[0] = PERSPECTIVE
    with pytest.raises(NotImplementedError, match="one type"):
        raygen.camera_rays(mixed, idx, coords)
    with pytest.raises(NotImplementedError, match="type 3"):
        raygen.camera_rays(cameras(g, cuda, EQUIRECTANGULAR), idx, coords)
    persp = cameras(g, cuda, PERSPECTIVE)
    with pytest.raises(NotImplementedError, match="undistort_perspective"):
        raygen.camera_rays(persp, idx, coords)
    assert raygen.camera_rays(persp, idx, coords, undistort_perspective=True).directions.shape == (512, 3)
    with pytest.raises(NotImplementedError, match="undistort_perspective"):  # the flag is not remembered
        raygen.camera_rays(persp, idx, coords)


def test_generated_bundle_drives_ray_order(g):
    from neurad_studio_amd import ops

    rb = run_case(g, "fisheye_rs")
    order = ops.ray_order(rb.origins, rb.directions, 100.0)
    assert order.shape == (512,) and sorted(order.tolist()) == list(range(512))
