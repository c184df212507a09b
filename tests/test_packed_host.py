"""Packed compositing, the part that needs no GPU: the C ABI declares and exports the entry points, their argument checks
run on the host before any launch, the tensor-level wrappers have no CPU path and the nerfacc shim's packed signatures
fail with the right exception."""
import ctypes

import pytest
import torch

from host_gate import header_functions

PACKED = ["nrhip_packed_segments", "nrhip_packed_weight_from_density", "nrhip_packed_weight_from_density_bwd",
          "nrhip_packed_weight_from_alpha", "nrhip_packed_weight_from_alpha_bwd", "nrhip_packed_accumulate",
          "nrhip_packed_accumulate_bwd", "nrhip_packed_composite_fwd", "nrhip_packed_composite_bwd"]
I32, I64 = ctypes.c_int32, ctypes.c_int64
ONE = ctypes.c_void_p(0x1000)  # any non-null address: validation fails before anything is dereferenced


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as ge
    from neurad_studio_amd import _lib

    if not os.path.exists(ge.LIB):
        ge.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_packed_entry_points(lib):
    from neurad_studio_amd import _lib

    fns = header_functions()
    for name in PACKED:
        assert name in fns, f"{name} is not declared in include/neurad_hip.h"
        assert name in _lib.PROTOTYPES
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.nrhip_version() >= 512


def _calls(r, seg, c=4, m=8):
    """every packed entry point with `r` rays, `seg` as the segments pointer and `c` channels; sample pointers non-null"""
    o = ONE
    return {
        "nrhip_packed_segments": (o, I64(m), I64(r), seg, None),
        "nrhip_packed_weight_from_density": (o, o, o, seg, I64(r), o, o, o, None),
        "nrhip_packed_weight_from_density_bwd": (o, o, o, seg, o, I64(r), o, None),
        "nrhip_packed_weight_from_alpha": (o, seg, I64(r), o, o, None),
        "nrhip_packed_weight_from_alpha_bwd": (o, seg, o, None, I64(r), o, None),
        "nrhip_packed_accumulate": (o, o, seg, I64(r), I32(c), o, None),
        "nrhip_packed_accumulate_bwd": (o, o, o, seg, I64(r), I32(c), o, o, None),
        "nrhip_packed_composite_fwd": (o, o, o, o, seg, I64(r), I32(c), I32(1), o, o, o, o, None),
        "nrhip_packed_composite_bwd": (o, o, o, o, seg, o, o, o, None, I64(r), I32(c), I32(1), o, o, None),
    }


def test_host_side_validation(lib):
    for name, args in _calls(-1, ONE).items():  # negative ray count
        assert getattr(lib, name)(*args) != 0, name
        assert b"negative" in lib.nrhip_last_error(), (name, lib.nrhip_last_error())
    for name, args in _calls(5, None).items():  # NULL segments
        assert getattr(lib, name)(*args) != 0, name
        assert b"segments" in lib.nrhip_last_error(), (name, lib.nrhip_last_error())
    assert lib.nrhip_packed_segments(ONE, I64(-1), I64(5), ONE, None) != 0  # negative sample count
    assert b"negative" in lib.nrhip_last_error()
    for name, args in _calls(5, ONE, c=0).items():  # c < 1
        if "accumulate" in name or "composite" in name:
            assert getattr(lib, name)(*args) != 0, name
            assert b"channel" in lib.nrhip_last_error(), (name, lib.nrhip_last_error())
    for mode in (2, -1):
        assert lib.nrhip_packed_composite_fwd(ONE, ONE, ONE, ONE, ONE, I64(5), I32(4), I32(mode), ONE, ONE, ONE, ONE, None) != 0
        assert b"mode" in lib.nrhip_last_error()
    assert lib.nrhip_packed_accumulate(ONE, None, ONE, I64(5), I32(3), ONE, None) != 0  # plain sum is one channel
    assert lib.nrhip_packed_accumulate(ONE, ONE, ONE, I64(5), I32(3), None, None) != 0  # no output


def test_zero_rays_is_a_no_op_with_every_pointer_null(lib):
    n = None
    assert lib.nrhip_packed_weight_from_density(n, n, n, n, I64(0), n, n, n, None) == 0
    assert lib.nrhip_packed_weight_from_density_bwd(n, n, n, n, n, I64(0), n, None) == 0
    assert lib.nrhip_packed_weight_from_alpha(n, n, I64(0), n, n, None) == 0
    assert lib.nrhip_packed_weight_from_alpha_bwd(n, n, n, n, I64(0), n, None) == 0
    assert lib.nrhip_packed_accumulate(n, n, n, I64(0), I32(1), n, None) == 0
    assert lib.nrhip_packed_accumulate_bwd(n, n, n, n, I64(0), I32(1), n, n, None) == 0
    assert lib.nrhip_packed_composite_fwd(n, n, n, n, n, I64(0), I32(3), I32(0), n, n, n, n, None) == 0
    assert lib.nrhip_packed_composite_bwd(n, n, n, n, n, n, n, n, n, I64(0), I32(3), I32(0), n, n, None) == 0


def test_wrappers_refuse_cpu_tensors():
    from neurad_studio_amd import _lib, ops

    M, R, C = 6, 3, 4
    z = torch.zeros
    seg = torch.tensor([0, 2, 2, 6])
    calls = [lambda: ops.packed_segments(z(M, dtype=torch.int64), R),
             lambda: ops.packed_weight_from_density(z(M), z(M), z(M), seg),
             lambda: ops.packed_weight_from_density_bwd(z(M), z(M), z(M), seg, z(M)),
             lambda: ops.packed_weight_from_alpha(z(M), seg),
             lambda: ops.packed_weight_from_alpha_bwd(z(M), seg, z(M), z(M)),
             lambda: ops.packed_accumulate(z(M), z(M, C), seg),
             lambda: ops.packed_accumulate(z(M), None, seg),
             lambda: ops.packed_accumulate_bwd(z(M), z(M, C), z(R, C), seg),
             lambda: ops.packed_composite_fwd(z(M), z(M), z(M), z(M, C), seg, True),
             lambda: ops.packed_composite_bwd(z(M), z(M), z(M), z(M, C), seg, False, z(R, C))]
    for k, fn in enumerate(calls):
        with pytest.raises(_lib.NeuradHipError):
            fn()
            pytest.fail(f"call {k} computed on CPU tensors")


def test_shim_packed_signatures_fail_with_the_right_exception():
    from neurad_studio_amd.model_components.renderers import render_packed
    from neurad_studio_amd.shims import nerfacc

    w, v, ri = torch.rand(6), torch.rand(6, 3), torch.tensor([0, 0, 1, 1, 1, 2])
    with pytest.raises(ValueError):  # packed ray_indices need n_rays
        nerfacc.accumulate_along_rays(w, v, ray_indices=ri)
    with pytest.raises(ValueError):
        nerfacc.render_weight_from_alpha(w, ray_indices=ri)
    with pytest.raises(ValueError):
        nerfacc.render_weight_from_density(w, w, w, ray_indices=ri)
    with pytest.raises(NotImplementedError):  # out of scope, and said so
        nerfacc.render_weight_from_alpha(w, ray_indices=ri, n_rays=3, prefix_trans=w)
    with pytest.raises(ValueError):
        nerfacc.pack_info(ri)
    with pytest.raises(ValueError):  # exactly one of density / alpha
        render_packed(v, None, ri, 3)
    with pytest.raises(ValueError):
        render_packed(v, None, ri, 3, density=w, alpha=w)


# ---- the nrhip_packed_rays descriptor: the same bad descriptor to every entry point that takes one -------------------
F32 = ctypes.c_float
INVALID_ARG, UNSUPPORTED = 1, 2  # NRHIP_ERR_INVALID_ARG, NRHIP_ERR_UNSUPPORTED
RAY_POINTERS = ("origins", "directions", "pixel_area", "t_starts", "t_ends", "segments")


def _field():
    """an nrhip_field the validation accepts; every pointer is the same non-null address"""
    from neurad_studio_amd import _lib

    f = _lib.Field()
    g = f.grid
    g.num_levels, g.n_features, g.log2_table_size, g.param_dtype = 8, 4, 11, 0
    for l in range(8):
        g.scalings[l] = 16.0 * 2 ** l
    f.table, f.static_scale, f.use_sdf, f.beta = 0x1000, 100.0, 1, 3.0
    f.geo.in_dim, f.geo.hidden_dim, f.geo.out_dim, f.geo.num_layers = 32, 32, 33, 2
    f.feat.in_dim, f.feat.hidden_dim, f.feat.out_dim, f.feat.num_layers = 48, 32, 32, 3
    for k in range(3):
        f.geo.weight[k] = f.geo.bias[k] = f.feat.weight[k] = f.feat.bias[k] = 0x1000
    return f


def _packed_rays(r, m, null=None):
    from neurad_studio_amd import _lib

    p = _lib.PackedRays()
    p.n_rays, p.n_samples = r, m
    for name in RAY_POINTERS:
        setattr(p, name, None if name == null else 0x1000)
    return p


def _descriptor_calls(lib, workspace_bytes=1 << 20):
    """name in the messages -> call(rays): the five entry points that take an nrhip_packed_rays, every other argument valid"""
    f, o = _field(), ONE
    return {
        "render_fwd_packed": lambda rays: lib.nrhip_render_fwd_packed(f, rays, o, o, o, o, F32(0.0), None),
        "field_fwd_train_packed": lambda rays: lib.nrhip_field_fwd_train_packed(f, rays, *(o,) * 7, None),
        "encode_bwd_rays_packed": lambda rays: lib.nrhip_encode_bwd_rays_packed(f.grid, o, F32(100.0), rays, o, I32(0), o, o, None),
        "encode_bwd_binned_packed": lambda rays: lib.nrhip_encode_bwd_binned_packed(
            f.grid, F32(100.0), rays, o, o, o, I32(1), o, I64(workspace_bytes), None),
        "encode_bwd_binned_packed_f16": lambda rays: lib.nrhip_encode_bwd_binned_packed_f16(
            f.grid, F32(100.0), rays, o, o, o, o, I64(workspace_bytes), None),
    }


def test_every_descriptor_entry_point_refuses_the_same_bad_descriptor(lib):
    """NULL descriptor, negative R, negative M, M = 2^31: the code, and the entry point's own name in the message."""
    err = lib.nrhip_last_error
    for who, call in _descriptor_calls(lib).items():
        for rays, code, fragment in ((None, INVALID_ARG, b"NULL"), (_packed_rays(-1, 8), INVALID_ARG, b"negative"),
                                     (_packed_rays(4, -8), INVALID_ARG, b"negative"),
                                     (_packed_rays(4, 1 << 31), UNSUPPORTED, b"2^31")):
            assert call(rays) == code, (who, fragment)
            assert err().startswith(who.encode() + b":") and fragment in err(), (who, err())


def test_every_descriptor_entry_point_names_itself_for_a_null_ray_pointer(lib):
    """One NULL pointer of the descriptor at a time, at R = 4, M = 8.  The binned pair finds a sample's ray through ray_of and
    never reads the segments: with NULL segments it goes on to its next check, which a 16-byte workspace fails (so that
    nothing is launched on the placeholder addresses)."""
    err = lib.nrhip_last_error
    for null in RAY_POINTERS:
        for who, call in _descriptor_calls(lib, workspace_bytes=16).items():
            assert call(_packed_rays(4, 8, null=null)) == INVALID_ARG, (who, null)
            want = b"workspace" if (null == "segments" and "binned" in who) else b"NULL pointer"
            assert err().startswith(who.encode() + b":") and want in err(), (who, null, err())
