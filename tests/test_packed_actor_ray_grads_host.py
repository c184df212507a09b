"""Ray gradients through the pair positions of packed samples, the part that needs no GPU: the helpers' scenes are what the
GPU tests take them for, the entry point is declared, prototyped and exported and checks its arguments on the host, the
wrapper has no CPU path, and the two new opt-ins default to off and leave the refusals in place."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import actor_refs as AR
import packed_actor_ray_grad_refs as RG
import packed_restatement as PR
from host_gate import header_functions, run_child

NAME = "nrhip_actor_pair_positions_bwd_rays_packed"
I32, I64 = ctypes.c_int32, ctypes.c_int64
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


# ---- the helpers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [16, 32, 64])
def test_exact_case_is_the_float64_chain_and_sits_on_the_groups_boundaries(G):
    from grad_edge_refs import actor_pair_grads64

    c = RG.exact_case(G)
    o, d, area, times, t0, t1, seg, flip = c["rays"]
    si, ai, gx, gs = c["pairs"]
    counts = np.diff(seg)
    n = c["n_pairs"]
    assert n.tolist() == [max(k, 0) for k in RG.exact_counts(G)]
    assert {0, 1, G - 1, G, G + 1, 2 * G + 1, 190} <= set(n.tolist())
    assert n[0] > 0 and n[-1] > 0 and si[0] >= seg[0] and si[-1] < seg[-1]
    empty = np.nonzero(counts == 0)[0]
    assert len(empty) and all(n[r - 1] > 0 and n[r + 1] > 0 for r in empty)      # no samples, between two rays with pairs
    assert ((counts > 0) & (n == 0)).any()                                       # samples, but no pair
    assert (np.diff(si) >= 0).all() and (np.bincount(si) == 2).any() and (np.bincount(si) == 3).any()
    # the closed form the case states is the float64 autograd of the whole chain, one pair at a time
    args, ray = RG.exact_as_dense(c)
    per = actor_pair_grads64(*args)
    assert (per["mag"] < 1).all()
    for key in ("go", "gd"):
        acc = np.zeros_like(c[key])
        np.add.at(acc, ray, per[key])
        assert np.allclose(acc, c[key], rtol=1e-12, atol=1e-12), key
        assert (np.abs(c[key][n > 0]).sum(-1) > 0).all() and (c[key][n == 0] == 0).all()


@pytest.mark.parametrize("kw,random_pairs", [(dict(seed=2), False), (dict(seed=2, scale=1.5), True), (dict(seed=1, wide=True), False)],
                         ids=["mag<1", "mag>1", "wide"])
def test_generic_scenes_keep_a_few_hundred_pairs_through_the_cut(kw, random_pairs):
    sc = AR.generic_scene(**kw)
    R, S = sc["starts"].shape
    si, ai = RG.random_sorted_pairs(sc) if random_pairs else RG.production_pairs(sc)
    assert (np.diff(si) >= 0).all()
    rays, keep, psi = RG.cut(sc, si, ai)
    assert keep.all() and np.array_equal(psi, si) and rays[4].shape == (R * S,)
    counts = RG.cut_counts(R)
    rays, keep, psi = RG.cut(sc, si, ai, counts)
    assert (counts == 0).any() and np.array_equal(np.diff(rays[6]), counts) and rays[4].shape == (counts.sum(),)
    assert keep.sum() >= 200 and (np.diff(psi) >= 0).all()
    ri = PR.ray_indices_from_segments(rays[6])
    assert np.array_equal(ri[psi], si[keep] // S)
    assert np.array_equal(rays[4][psi], sc["starts"].reshape(-1)[si[keep]])


def test_take_rays_keeps_every_pair_with_its_ray():
    c = RG.exact_case(16)
    R = len(c["n_pairs"])
    perm = np.random.default_rng(5).permutation(R)
    rays, pairs, frm = RG.take_rays(c["rays"], c["pairs"], perm)
    assert np.array_equal(np.sort(frm), np.arange(len(frm))) and (np.diff(pairs[0]) >= 0).all()
    ri = PR.ray_indices_from_segments(rays[6])
    assert np.array_equal(np.bincount(ri[pairs[0]], minlength=R), c["n_pairs"][perm])
    assert np.array_equal(rays[4][pairs[0]], c["rays"][4][c["pairs"][0][frm]])
    half, pairs_h, frm_h = RG.take_rays(c["rays"], c["pairs"], np.arange(0, R, 2))
    assert len(frm_h) == c["n_pairs"][::2].sum() and half[0].shape[0] == (R + 1) // 2


# ---- the entry point -----------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point(lib):
    from neurad_studio_amd import _lib

    assert NAME in header_functions(), f"{NAME} is not declared in include/neurad_hip.h"
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME]) == 13
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert lib.nrhip_version() == 520


def _actors():
    from neurad_studio_amd import _lib

    a = _lib.Actors()
    a.n_times, a.n_actors, a.actor_scale, a.max_candidates = 2, 3, 10.0, 3
    a.timestamps = a.positions = a.rotations_6d = a.present = a.bounds = a.tables = 0x1000
    return a


def _rays(r, m, ptr=0x1000, seg=0x1000):
    from neurad_studio_amd import _lib

    p = _lib.PackedRays()
    p.n_rays, p.n_samples = r, m
    p.origins = p.directions = p.pixel_area = p.t_starts = p.t_ends = ptr
    p.segments = seg
    return p


def test_host_side_validation(lib):
    a, o, n = _actors(), ONE, None
    err = lib.nrhip_last_error

    def call(rays, p=5, ins=(o,) * 5, lanes=0, out=(o, o), actors=a):
        times, si, ai, gx, gc = ins
        return getattr(lib, NAME)(actors, rays, times, si, ai, None, I64(p), gx, gc, I32(lanes), *out, None)

    assert call(_rays(4, 8), actors=None) == INVALID_ARG
    assert call(None) == INVALID_ARG
    assert call(_rays(-1, 8)) == INVALID_ARG and b"negative" in err()
    assert call(_rays(4, -8)) == INVALID_ARG and b"negative" in err()
    assert call(_rays(4, 1 << 31)) == UNSUPPORTED and b"2^31" in err()
    assert call(_rays(4, 8), p=-1) == INVALID_ARG
    for lanes in (1, 8, 17, 48, 128, -16):
        assert call(_rays(4, 8), lanes=lanes) == INVALID_ARG and b"lanes_per_ray" in err(), lanes
    for rays in (_rays(0, 0, ptr=None, seg=None), _rays(4, 0, ptr=None, seg=None)):
        assert call(rays, p=5) == INVALID_ARG and b"without samples" in err()
    for out in ((n, o), (o, n)):
        assert call(_rays(4, 8), out=out) == INVALID_ARG and b"NULL pointer" in err()
        assert call(_rays(4, 8), p=0, out=out) == INVALID_ARG and b"NULL pointer" in err()
    for k in range(5):
        ins = [o] * 5
        ins[k] = n
        assert call(_rays(4, 8), ins=ins) == INVALID_ARG and b"NULL pointer" in err(), k
    assert call(_rays(4, 8, ptr=None)) == INVALID_ARG and b"NULL pointer" in err()
    assert call(_rays(4, 8, seg=None)) == INVALID_ARG and b"NULL pointer" in err()  # the segments are required here
    # no rays: a no-op that reads no pointer
    assert call(_rays(0, 0, ptr=None, seg=None), p=0, ins=(n,) * 5, out=(n, n)) == 0


def test_wrapper_checks_its_shapes_and_refuses_cpu_tensors():
    from neurad_studio_amd import _lib, ops

    z = torch.zeros
    o, d, a, t = z(2, 3), z(2, 3), z(2), z(2)
    ts, te, seg = z(4), z(4), torch.tensor([0, 2, 4])
    si, ai = torch.tensor([1]), torch.tensor([0], dtype=torch.int32)
    for lanes in (0, 16, 32, 64):
        with pytest.raises(_lib.NeuradHipError, match="GPU tensor"):
            ops.actor_pair_positions_packed_bwd_rays(None, o, d, a, ts, te, seg, t, si, ai, None, z(1, 3), z(1), lanes_per_ray=lanes)
    p = inspect.signature(ops.actor_pair_positions_packed_bwd_rays).parameters
    assert p["lanes_per_ray"].default == 0
    # the sibling's signature is as it was
    assert list(inspect.signature(ops.actor_pair_positions_packed_bwd).parameters) == [
        "spec", "origins", "directions", "pixel_area", "t_starts", "t_ends", "ray_indices", "times", "sample_idx", "actor_idx",
        "ray_flip", "grad_x01", "grad_cstd"]


def test_pair_samples_without_segments_refuse_rays_that_require_grad():
    from neurad_studio_amd import autograd as ag

    z = torch.zeros
    s = ag.PackedSamples(z(4), z(4), ray_indices=torch.tensor([0, 0, 1, 1]))
    with pytest.raises(ValueError, match="segments"):
        s.pair_positions_bwd(None, z(2, 3), z(2, 3), z(2), z(2), torch.tensor([1]), torch.tensor([0], dtype=torch.int32), None,
                             z(1, 3), z(1), True, False)
    p = inspect.signature(ag.ActorPairPositionsFn.forward).parameters
    assert list(p)[-2:] == ["ray_indices", "segments"] and p["segments"].default is None


# ---- the gates -----------------------------------------------------------------------------------------------------------
GATES_CHILD = r'''
import inspect
from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler


def raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return [type(e).__name__, str(e)]
    return None


out = {"defaults": [inspect.signature(NeuRADField.render_train_packed).parameters["actor_ray_gradients"].default,
                    inspect.signature(VolumetricSampler.render_train).parameters["fused_actor_ray_gradients"].default]}
z = torch.zeros
fld = NeuRADField(field_config(8, 4, 32), actors=make_actors(), static_scale=100.0).train()
d, a, t, ts, te = z(2, 3), z(2), z(2), z(4), z(4)
seg = torch.tensor([0, 2, 4])
og = lambda: z(2, 3, requires_grad=True)
call = fld.render_train_packed
out["default"] = raised(lambda: call(og(), d, a, ts, te, segments=seg, times=t))
out["false"] = raised(lambda: call(og(), d, a, ts, te, segments=seg, times=t, actor_ray_gradients=False))
out["static flag"] = raised(lambda: call(og(), d, a, ts, te, segments=seg, times=t, ray_gradients=True))
# opted in, the refusal is gone: the call reaches the device check of the first wrapper (CPU tensors here)
out["true"] = raised(lambda: call(og(), d, a, ts, te, segments=seg, times=t, actor_ray_gradients=True))
out["true, d"] = raised(lambda: call(z(2, 3), og(), a, ts, te, segments=seg, times=t, actor_ray_gradients=True))
# the flag does not open the static refusals: no times on an actor field; a static field whose rays move
out["no times"] = raised(lambda: call(og(), d, a, ts, te, segments=seg, actor_ray_gradients=True))
static = NeuRADField(field_config(8, 4, 32), actors=None, static_scale=100.0).train()
out["static field"] = raised(lambda: static.render_train_packed(og(), d, a, ts, te, segments=seg, actor_ray_gradients=True))
print(json.dumps(out))
'''


def test_opt_ins_default_to_off_and_leave_the_refusals_in_place():
    out = run_child(GATES_CHILD)
    assert out["defaults"] == [False, False]
    for key in ("default", "false", "static flag"):
        kind, text = out[key]
        assert kind == "NotImplementedError", (key, out[key])
        assert "no gradient reaches the rays through the actor branch on packed samples" in text and "operator route" in text
        assert "rays" in text and "actor" in text
    for key in ("true", "true, d"):
        assert out[key] and out[key][0] == "NeuradHipError", (key, out[key])  # past every gate: the missing device stops it
    for key in ("no times", "static field"):
        assert out[key][0] == "NotImplementedError" and "operator route" in out[key][1], (key, out[key])
    assert "no gradient reaches the rays through packed samples" in out["static field"][1]
