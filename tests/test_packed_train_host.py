"""Training on packed samples, the part that needs no GPU: the C ABI declares and exports the six entry points, their
argument checks run on the host before any launch, the tensor-level wrappers have no CPU path, and the field's gate and
argument checks answer without a device."""
import ctypes

import pytest
import torch

from host_gate import header_functions, run_child

NEW = ["nrhip_field_fwd_train_packed", "nrhip_sdf_render_packed_fwd", "nrhip_sdf_render_packed_bwd_workspace",
       "nrhip_sdf_render_packed_bwd", "nrhip_encode_bwd_binned_packed", "nrhip_encode_bwd_binned_packed_f16"]
I32, I64, F32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
ONE = ctypes.c_void_p(0x1000)  # any non-null address: validation fails before anything is dereferenced
INVALID_ARG, UNSUPPORTED = 1, 2  # NRHIP_ERR_INVALID_ARG, NRHIP_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as ge
    from neurad_studio_amd import _lib

    if not os.path.exists(ge.LIB):
        ge.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from neurad_studio_amd import _lib

    fns = header_functions()
    for name in NEW:
        assert name in fns, f"{name} is not declared in include/neurad_hip.h"
        assert name in _lib.PROTOTYPES
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.nrhip_version() >= 515


def _field(L=8, F=4, H=32):
    """an nrhip_field the validation accepts; every pointer is the same non-null address"""
    from neurad_studio_amd import _lib

    f = _lib.Field()
    g = f.grid
    g.num_levels, g.n_features, g.log2_table_size, g.param_dtype = L, F, 11, 0
    for l in range(L):
        g.scalings[l] = 16.0 * 2 ** l
    f.table, f.static_scale, f.use_sdf, f.beta = 0x1000, 100.0, 1, 3.0
    f.geo.in_dim, f.geo.hidden_dim, f.geo.out_dim, f.geo.num_layers = L * F, H, 33, 2
    f.feat.in_dim, f.feat.hidden_dim, f.feat.out_dim, f.feat.num_layers = 48, H, 32, 3
    for k in range(3):
        f.geo.weight[k] = f.geo.bias[k] = f.feat.weight[k] = f.feat.bias[k] = 0x1000
    return f


def _rays(r, m, ptr=0x1000, seg=0x1000):
    from neurad_studio_amd import _lib

    p = _lib.PackedRays()
    p.n_rays, p.n_samples = r, m
    p.origins = p.directions = p.pixel_area = p.t_starts = p.t_ends = ptr
    p.segments = seg
    return p


def _err(lib):
    return lib.nrhip_last_error()


def test_host_side_validation(lib):
    f, o = _field(), ONE
    fwd_train = lambda rays, *out: lib.nrhip_field_fwd_train_packed(f, rays, *out, None)  # noqa: E731
    seven = (o,) * 7
    # negative counts
    assert fwd_train(_rays(-1, 8), *seven) == INVALID_ARG and b"negative" in _err(lib)
    assert fwd_train(_rays(4, -8), *seven) == INVALID_ARG and b"negative" in _err(lib)
    # M >= 2^31
    assert fwd_train(_rays(4, 1 << 31), *seven) == UNSUPPORTED and b"2^31" in _err(lib)
    # a NULL output, every position
    for k in range(7):
        out = [o] * 7
        out[k] = None
        assert fwd_train(_rays(4, 8), *out) == INVALID_ARG and b"NULL output" in _err(lib), k
    # unaligned save buffer (the dense entry point's check)
    assert fwd_train(_rays(4, 8), o, o, o, ctypes.c_void_p(0x1004), o, o, o) == INVALID_ARG and b"aligned" in _err(lib)
    # NULL segments / ray pointer
    assert fwd_train(_rays(4, 8, seg=None), *seven) == INVALID_ARG and b"NULL pointer" in _err(lib)
    assert fwd_train(_rays(4, 8, ptr=None), *seven) == INVALID_ARG and b"NULL pointer" in _err(lib)
    assert lib.nrhip_field_fwd_train_packed(f, None, *seven, None) == INVALID_ARG

    head_fwd = lambda r, seg, c, outs=(o,) * 5: lib.nrhip_sdf_render_packed_fwd(  # noqa: E731
        o, o, F32(1e-4), o, o, o, seg, I64(r), I32(c), *outs, None)
    head_bwd = lambda r, seg, c, outs=(o, o, o, o): lib.nrhip_sdf_render_packed_bwd(  # noqa: E731
        o, o, F32(1e-4), o, o, o, o, seg, o, o, o, o, I64(r), I32(c), *outs, None)
    for call in (head_fwd, head_bwd):
        assert call(-1, o, 32) == INVALID_ARG and b"negative" in _err(lib)
        assert call(5, None, 32) == INVALID_ARG and b"segments" in _err(lib)
        assert call(5, o, 0) == INVALID_ARG and b"channel" in _err(lib)
    for k in (2, 3, 4):  # the per-ray outputs
        outs = [o] * 5
        outs[k] = None
        assert head_fwd(5, o, 32, outs) == INVALID_ARG and b"NULL" in _err(lib)
    for k in range(4):  # grad_features, grad_geo_out, grad_beta (SDF head), workspace
        outs = [o] * 4
        outs[k] = None
        assert head_bwd(5, o, 32, outs) == INVALID_ARG and b"NULL" in _err(lib), k
    n = I64(0)
    assert lib.nrhip_sdf_render_packed_bwd_workspace(I64(-1), ctypes.byref(n)) == INVALID_ARG
    assert lib.nrhip_sdf_render_packed_bwd_workspace(I64(5), None) == INVALID_ARG
    assert lib.nrhip_sdf_render_packed_bwd_workspace(I64(9001), ctypes.byref(n)) == 0 and n.value >= 1

    g = f.grid
    enc = lambda rays, ri=o, go=o, gt=o: lib.nrhip_encode_bwd_binned_packed(  # noqa: E731
        g, F32(100.0), rays, ri, go, gt, I32(1), o, I64(1 << 20), None)
    enc16 = lambda rays, ri=o, go=o, gt=o: lib.nrhip_encode_bwd_binned_packed_f16(  # noqa: E731
        g, F32(100.0), rays, ri, go, gt, o, I64(1 << 20), None)
    for call in (enc, enc16):
        assert call(_rays(-1, 8)) == INVALID_ARG and b"negative" in _err(lib)
        assert call(_rays(4, -8)) == INVALID_ARG and b"negative" in _err(lib)
        assert call(_rays(4, 1 << 31)) == UNSUPPORTED and b"2^31" in _err(lib)
        assert call(_rays(4, 8), gt=None) == INVALID_ARG
        assert call(_rays(4, 8), ri=None) == INVALID_ARG and b"NULL pointer" in _err(lib)
        assert call(_rays(4, 8, ptr=None)) == INVALID_ARG and b"NULL pointer" in _err(lib)
        assert call(None) == INVALID_ARG
    assert enc16(_rays(4, 0)) == INVALID_ARG and b"at least one sample" in _err(lib)
    # a workspace smaller than the query's answer is refused before any launch
    need = I64(0)
    assert lib.nrhip_encode_bwd_binned_workspace(g, I64(1 << 15), ctypes.byref(need)) == 0 and need.value > 16
    assert lib.nrhip_encode_bwd_binned_packed(g, F32(100.0), _rays(4, 1 << 15), o, o, o, I32(1), o, I64(16), None) == INVALID_ARG
    assert b"workspace" in _err(lib)


def test_zero_rays_is_a_no_op_with_every_pointer_null(lib):
    f, n = _field(), None
    seven = (n,) * 7
    assert lib.nrhip_field_fwd_train_packed(f, _rays(0, 0, ptr=None, seg=None), *seven, None) == 0
    assert lib.nrhip_field_fwd_train_packed(f, _rays(5, 0, ptr=None, seg=None), *seven, None) == 0  # no samples: nothing is read
    assert lib.nrhip_sdf_render_packed_fwd(n, n, F32(0), n, n, n, n, I64(0), I32(32), n, n, n, n, n, None) == 0
    assert lib.nrhip_sdf_render_packed_bwd(n, n, F32(0), n, n, n, n, n, n, n, n, n, I64(0), I32(32), n, n, n, n, None) == 0
    assert lib.nrhip_encode_bwd_binned_packed(f.grid, F32(100.0), _rays(0, 0, ptr=None, seg=None), n, n, ONE, I32(1), n, I64(0),
                                              None) == 0


def test_wrappers_refuse_cpu_tensors():
    from neurad_studio_amd import _lib, ops

    M, R, C = 6, 3, 32
    z = torch.zeros
    seg, ri = torch.tensor([0, 2, 2, 6]), torch.tensor([0, 0, 2, 2, 2, 2])
    spec = ops.GridSpec(8, 4, 11, 16, 1024)
    fs = ops.FieldSpec(spec, z(8 * 2**11, 4), 100.0, [z(32, 32), z(33, 32)], [z(32), z(33)], [z(32, 48), z(32, 32), z(32, 32)],
                       [z(32), z(32), z(32)], True, 3.0)
    calls = [lambda: ops.field_fwd_train_packed(fs, z(R, 3), z(R, 3), z(R), z(M), z(M), seg),
             lambda: ops.sdf_render_packed_fwd(z(M), z(1), 1e-4, z(M, C), z(M), z(M), seg),
             lambda: ops.sdf_render_packed_fwd(z(M), None, 0.0, z(M, C), z(M), z(M), seg),
             lambda: ops.sdf_render_packed_bwd(z(M), z(1), 1e-4, z(M), z(M, C), z(M), z(M), seg, z(R, C), z(R), z(R), z(M)),
             lambda: ops.encode_bwd_packed(spec, 100.0, z(R, 3), z(R, 3), z(R), z(M), z(M), ri, z(M, 32)),
             lambda: ops.packed_ray_indices(seg, M)]
    for k, fn in enumerate(calls):
        with pytest.raises(_lib.NeuradHipError):
            fn()
            pytest.fail(f"call {k} computed on CPU tensors")


GATE_CHILD = r'''
out = {}
for name, (L, F, H, actors) in {"8x4-H32": (8, 4, 32, False), "8x4-H32-actors": (8, 4, 32, True), "3x4-H32": (3, 4, 32, False),
                                "8x4-H48": (8, 4, 48, False)}.items():
    fld = NeuRADField(field_config(L, F, H), actors=make_actors() if actors else None, static_scale=100.0)
    out[name] = [fld.fused_packed_train_supported(), fld.fused_packed_supported() and fld._fused_train_ok()]
fld = NeuRADField(field_config(8, 4, 32), actors=None, static_scale=100.0)
z = torch.zeros
errs = []
for kw in ({}, {"segments": z(4, dtype=torch.int64), "ray_indices": z(6, dtype=torch.int64), "num_rays": 3},
           {"ray_indices": z(6, dtype=torch.int64)}):
    try:
        fld.render_train_packed(z(3, 3), z(3, 3), z(3), z(6), z(6), **kw)
        errs.append("none")
    except Exception as e:
        errs.append(type(e).__name__)
out["errors"] = errs
act = NeuRADField(field_config(8, 4, 32), actors=make_actors(), static_scale=100.0)
try:
    act.render_train_packed(z(3, 3), z(3, 3), z(3), z(6), z(6), segments=z(4, dtype=torch.int64))
    out["actors"] = "none"
except NotImplementedError as e:
    out["actors"] = str(e)
try:
    fld.render_train_packed(z(3, 3).requires_grad_(True), z(3, 3), z(3), z(6), z(6), segments=z(4, dtype=torch.int64))
    out["ray_grad"] = "none"
except NotImplementedError as e:
    out["ray_grad"] = str(e)
print(json.dumps(out))
'''


def test_gate_and_argument_checks_of_the_field():
    out = run_child(GATE_CHILD)
    assert out["8x4-H32"] == [True, True]
    assert out["8x4-H32-actors"] == [False, False]  # the occupancy route is static
    assert out["3x4-H32"] == [False, False] and out["8x4-H48"] == [False, False]  # shapes outside _FUSED_GRIDS / widths
    assert out["errors"] == ["ValueError", "ValueError", "ValueError"]  # neither, both, ray_indices without num_rays
    assert "operator route" in out["actors"] and "operator route" in out["ray_grad"]
