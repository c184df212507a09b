"""Ray generation with a lens, the part that needs no GPU: the C ABI declares and exports nrhip_camera_rays_lens, its
argument checks run on the host before any launch, camera_rays has no CPU path, and the committed fixture is what the
reference gives (scripts/make_golden_raygen_lens.py, where the reference is present)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import ref_import
from conftest import ROOT, load_golden
from host_gate import header_functions
from raygen_lens_cases import FISHEYE, case_inputs

I64 = ctypes.c_int64
ONE = 0x1000  # any non-null address: validation fails before anything is dereferenced
INVALID_ARG, UNSUPPORTED = 1, 2  # NRHIP_ERR_INVALID_ARG, NRHIP_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from neurad_studio_amd import _lib

    if not os.path.exists(ge.LIB):
        ge.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_entry_point(lib):
    from neurad_studio_amd import _lib

    assert "nrhip_camera_rays_lens" in header_functions() and "nrhip_camera_rays_lens" in _lib.PROTOTYPES
    assert hasattr(lib, "nrhip_camera_rays_lens")
    assert lib.nrhip_version() >= 517
    assert ctypes.sizeof(_lib.CameraLens) == 16  # int32 (+ pad), pointer


def _table():
    from neurad_studio_amd import _lib

    t = _lib.CameraTable()
    t.camera_to_worlds = t.fx = t.fy = t.cx = t.cy = ONE
    return t


def _lens(camera_type=FISHEYE):
    from neurad_studio_amd import _lib

    lens = _lib.CameraLens()
    lens.camera_type = camera_type
    return lens


def test_host_side_validation(lib):
    fn, err = lib.nrhip_camera_rays_lens, lib.nrhip_last_error
    rays = (ONE,) * 2  # camera_indices, coords
    outs = (ONE,) * 5 + (None,)  # five outputs, stream
    assert fn(_table(), None, *rays, I64(8), *outs) == INVALID_ARG and b"lens" in err()
    assert fn(None, _lens(), *rays, I64(8), *outs) == INVALID_ARG
    assert fn(_table(), _lens(3), *rays, I64(8), *outs) == UNSUPPORTED and b"camera type 3" in err()
    assert fn(_table(), _lens(0), *rays, I64(0), *outs) == UNSUPPORTED  # whatever the ray count
    assert fn(_table(), _lens(), *rays, I64(-1), *outs) == INVALID_ARG and b"negative" in err()
    assert fn(_table(), _lens(), None, None, I64(0), *(None,) * 6) == 0  # nothing to do, no pointer is looked at
    assert fn(_table(), _lens(), None, ONE, I64(8), *outs) == INVALID_ARG and b"NULL pointer" in err()
    t = _table()
    t.rolling_shutter = 1  # rolling shutter without its tables
    assert fn(t, _lens(), *rays, I64(8), *outs) == INVALID_ARG and b"rolling shutter" in err()
    t.rolling_shutter = 4
    assert fn(t, _lens(), *rays, I64(8), *outs) == INVALID_ARG and b"rolling_shutter mode" in err()


def test_camera_rays_refuses_cpu_tensors_past_the_gate():
    from neurad_studio_amd import _lib
    from neurad_studio_amd.cameras.raygen import camera_rays

    for case in ("fisheye", "fisheye_plain", "persp_dist"):  # the gate lets all three through; there is no CPU path behind it
        cams, idx, coords = case_inputs(load_golden("raygen_lens"), case, torch.from_numpy)
        with pytest.raises(_lib.NeuradHipError, match="no CPU fallback"):
            camera_rays(cams, idx, coords, undistort_perspective=True)


@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
def test_committed_fixture_is_what_the_reference_gives():
    spec = importlib.util.spec_from_file_location("make_golden_raygen_lens",
                                                  os.path.join(ROOT, "scripts", "make_golden_raygen_lens.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh, committed = gen.generate(), load_golden("raygen_lens")
    assert set(fresh) == set(committed)
    for k, v in fresh.items():
        assert v.dtype == committed[k].dtype and v.shape == committed[k].shape, k
        assert v.tobytes() == committed[k].tobytes(), f"{k}: the committed fixture is not what the generator gives"
