"""Ray gradients through packed samples, the part that needs no GPU: the helper's reference is the oracle's function, the
entry point is declared, prototyped and exported and checks its arguments on the host, the wrapper has no CPU path, and
the field's opt-in leaves the default refusal in place."""
import ctypes

import numpy as np
import pytest
import torch

import neurad_oracle as O
import packed_ray_grad_refs as G
import packed_restatement as PR
import synth
from host_gate import header_functions, run_child

NAME = "nrhip_encode_bwd_rays_packed"
I32, F32 = ctypes.c_int32, ctypes.c_float
ONE = ctypes.c_void_p(0x1000)  # any non-null address: validation fails before anything is dereferenced
INVALID_ARG, UNSUPPORTED = 1, 2


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as ge
    from neurad_studio_amd import _lib

    if not os.path.exists(ge.LIB):
        ge.build()
    return _lib.load()


@pytest.mark.parametrize("S", [1, 5])
def test_reference_on_uniform_segments_is_the_oracle_on_the_dense_batch(S):
    R, F = 9, 4
    o, d, area, _ = synth.rays(R, 13)
    _, eu, _ = O.power_sampler(np.zeros(R), np.full(R, 300.0, np.float32), S)
    st, en = eu[:, :-1].copy(), eu[:, 1:].copy()
    grid = G.grid_for(F, False)
    ge = G.sharp_gradients(R * S, 32, 40 + S, 1.0)
    want = O.encode_static_ray_grads(grid, G.STATIC_SCALE, o, d, area, st, en, ge, with_abs=True)
    rays = (o, d, area, st.reshape(-1), en.reshape(-1), PR.segments_from_counts([S] * R))
    got = G.reference(grid, G.STATIC_SCALE, rays, ge)
    for g_, w_, A in zip(got[:2], want[:2], want[2:]):   # float64 rounding of sums of S terms, against their |terms|
        assert (np.abs(g_ - w_) <= 4 * S * 2.0**-52 * A).all()
    for g_, w_ in zip(got[2:], want[2:]):
        assert np.allclose(g_, w_, rtol=4 * S * 2.0**-52, atol=0)


def test_reference_gives_zero_to_rays_without_samples_and_gamma_follows_the_ray():
    counts = (0, 3, 0, 40, 0)
    o, d, area, _ = synth.rays(5, 17)
    seg = PR.segments_from_counts(counts)
    rng = np.random.default_rng(2)
    ts = np.concatenate([np.sort(rng.uniform(0.1, 60, n)) for n in counts]).astype(np.float32)
    ge = G.sharp_gradients(43, 32, 5, 1.0)
    ref = G.reference(G.grid_for(4, False), G.STATIC_SCALE, (o, d, area, ts, ts + np.float32(0.5), seg), ge)
    for a in ref:
        assert a.shape == (5, 3) and (a[[0, 2, 4]] == 0).all() and (a[[1, 3]] != 0).all()
    assert G.gamma(counts, 16, 8, 4)[:, 0].tolist() == [64, 65, 64, 67, 64]
    assert G.gamma(counts, 64, 8, 4)[:, 0].tolist() == [66, 67, 66, 67, 66]
    assert G.chosen_group(43, 5) == 16 and G.chosen_group(81, 5) == 32 and G.chosen_group(161, 5) == 64
    assert (G.gamma(counts, 0, 8, 4) == G.gamma(counts, 16, 8, 4)).all()
    empty = G.reference(G.grid_for(4, False), G.STATIC_SCALE, (o, d, area, ts[:0], ts[:0], np.zeros(6, np.int64)), ge[:0])
    assert all((a == 0).all() for a in empty)


def test_ragged_batch_has_samples_on_both_sides_of_the_contraction():
    import packed_train_refs as T

    o, d, area, ts, te, seg = T.packed_rays(T.RAGGED, 7)
    ri = PR.ray_indices_from_segments(seg)
    mid = o[ri] + d[ri] * ((ts + te) / 2)[:, None]
    mag = np.abs(mid / G.STATIC_SCALE).max(-1)
    assert (mag < 1).sum() > 100 and (mag >= 1).sum() > 100


def test_header_declares_and_library_exports_the_entry_point(lib):
    from neurad_studio_amd import _lib

    assert NAME in header_functions(), f"{NAME} is not declared in include/neurad_hip.h"
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME]) == 9
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert lib.nrhip_version() >= 516


def _grid(F=4):
    from neurad_studio_amd import _lib

    g = _lib.Grid()
    g.num_levels, g.n_features, g.log2_table_size, g.param_dtype = 8, F, 11, 0
    for l in range(8):
        g.scalings[l] = 16.0 * 2 ** l
    return g


def _rays(r, m, ptr=0x1000, seg=0x1000):
    from neurad_studio_amd import _lib

    p = _lib.PackedRays()
    p.n_rays, p.n_samples = r, m
    p.origins = p.directions = p.pixel_area = p.t_starts = p.t_ends = ptr
    p.segments = seg
    return p


def test_host_side_validation(lib):
    g, o = _grid(), ONE
    call = lambda rays, table=o, scale=100.0, go=o, lanes=0, out=(o, o): getattr(lib, NAME)(  # noqa: E731
        g, table, F32(scale), rays, go, I32(lanes), *out, None)
    err = lib.nrhip_last_error
    assert call(None) == INVALID_ARG
    assert call(_rays(-1, 8)) == INVALID_ARG and b"negative" in err()
    assert call(_rays(4, -8)) == INVALID_ARG and b"negative" in err()
    assert call(_rays(4, 1 << 31)) == UNSUPPORTED and b"2^31" in err()
    assert call(_rays(0, 8)) == INVALID_ARG and b"without rays" in err()
    for scale in (0.0, -1.0):
        assert call(_rays(4, 8), scale=scale) == INVALID_ARG and b"scale" in err()
    for lanes in (1, 8, 17, 48, 128, -16):
        assert call(_rays(4, 8), lanes=lanes) == INVALID_ARG and b"lanes_per_ray" in err(), lanes
    for out in ((None, o), (o, None)):
        assert call(_rays(4, 8), out=out) == INVALID_ARG and b"NULL output" in err()
        assert call(_rays(4, 0), out=out) == INVALID_ARG and b"NULL output" in err()
    assert call(_rays(4, 8), table=None) == INVALID_ARG and b"NULL pointer" in err()
    assert call(_rays(4, 8), go=None) == INVALID_ARG and b"NULL pointer" in err()
    assert call(_rays(4, 8, ptr=None)) == INVALID_ARG and b"NULL pointer" in err()
    assert call(_rays(4, 8, seg=None)) == INVALID_ARG and b"NULL pointer" in err()
    # no rays: a no-op that reads no pointer
    assert call(_rays(0, 0, ptr=None, seg=None), table=None, go=None, out=(None, None)) == 0


def test_wrapper_checks_the_gradient_size_and_refuses_cpu_tensors():
    from neurad_studio_amd import _lib, ops

    M, R = 6, 3
    z = torch.zeros
    seg = torch.tensor([0, 2, 2, 6])
    spec = ops.GridSpec(8, 4, 11, 16, 1024)
    args = (spec, z(8 * 2**11, 4), 100.0, z(R, 3), z(R, 3), z(R), z(M), z(M), seg)
    for bad in (z(M, 31), z(M - 1, 32), z(0)):
        with pytest.raises(ValueError, match="grad_out"):
            ops.encode_bwd_rays_packed(*args, bad)
    for lanes in (0, 16, 32, 64):
        with pytest.raises(_lib.NeuradHipError):
            ops.encode_bwd_rays_packed(*args, z(M, 32), lanes_per_ray=lanes)
            pytest.fail("computed on CPU tensors")


OPT_IN_CHILD = r'''
import inspect
from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
fld = NeuRADField(field_config(8, 4, 32), actors=None, static_scale=100.0)
z = torch.zeros
out = {"defaults": [inspect.signature(NeuRADField.render_train_packed).parameters["ray_gradients"].default,
                    inspect.signature(VolumetricSampler.render_train).parameters["fused_ray_gradients"].default]}
for key, kw in (("default", {}), ("false", {"ray_gradients": False})):
    try:
        fld.render_train_packed(z(3, 3), z(3, 3).requires_grad_(True), z(3), z(6), z(6), segments=z(4, dtype=torch.int64), **kw)
        out[key] = "none"
    except NotImplementedError as e:
        out[key] = str(e)
# opted in, the refusal is gone: the call reaches the device check of the first wrapper (CPU tensors here)
try:
    fld.render_train_packed(z(3, 3).requires_grad_(True), z(3, 3), z(3), z(6), z(6), segments=z(4, dtype=torch.int64),
                            ray_gradients=True)
    out["true"] = "none"
except NotImplementedError as e:
    out["true"] = "NotImplementedError: " + str(e)
except Exception as e:
    out["true"] = type(e).__name__
act = NeuRADField(field_config(8, 4, 32), actors=make_actors(), static_scale=100.0)
try:
    act.render_train_packed(z(3, 3), z(3, 3), z(3), z(6), z(6), segments=z(4, dtype=torch.int64), ray_gradients=True)
    out["actors"] = "none"
except NotImplementedError as e:
    out["actors"] = str(e)
print(json.dumps(out))
'''


def test_the_fields_opt_in_leaves_the_default_refusal_in_place():
    out = run_child(OPT_IN_CHILD)
    assert out["defaults"] == [False, False]
    for key in ("default", "false"):
        assert "no gradient reaches the rays through packed samples" in out[key] and "operator route" in out[key]
    assert out["true"] == "NeuradHipError"          # past every gate, stopped only by the missing device
    assert "operator route" in out["actors"]         # the actor gate is unchanged by the flag
