"""CPU checks of the surface normals in a scene with dynamic actors (csrc/normals.hip; the contract: include/neurad_hip.h at
nrhip_field_normals_actors): the conditions the GPU tests' scene must meet, from the oracle alone; the numpy restatement of
tests/normals_actor_refs.py on the oracle's own primal against the reference's autograd (tests/golden/normals_actors.npz,
made by scripts/make_golden_normals_actors.py) at the project's parity bar, rel-L2 <= 1e-4, in-box samples and the rest
separately; four wrong chains the golden tells apart; and the host-side argument checks of the two entry points."""
import ctypes
import functools
import os

import numpy as np
import pytest

import normals_actor_refs as AR
import normals_refs as NR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normals_actors.npz")
PARITY = 1e-4  # BASELINE north star: rel-L2 against the reference


@functools.lru_cache(maxsize=None)
def oracle_case(name, flip=False, edit=False):
    p, ap = AR.case_params(name)
    return p, ap, AR.oracle_restatement(p, ap, ray_flip=AR.ray_flips() if flip else None, edit=AR.EDIT if edit else None)


# ---- the scene ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flip,edit", [(n, False, False) for n in AR.CASES]
                         + [("8x4_h32_sdf", True, False), ("8x4_h32_sdf", False, True)])
def test_scene_conditions_of_the_gpu_cases(name, flip, edit):
    """every case the GPU tests use: >= 15 % of the samples in a box, a sample inside two boxes, a ray without candidates, and
    at most 1 % left out (a ReLU mask or a box face within rounding)"""
    p, ap, r = oracle_case(name, flip, edit)
    sc = AR.scene()
    assert (r["hit"] >= 0).mean() >= 0.15
    assert (r["n_boxes"] >= 2).sum() >= 1
    two = r["n_boxes"] >= 2
    assert (r["hit"][two] == 2).all()  # actors 1 and 2 overlap: the winner is the higher index
    cand = AR.candidates(ap, *AR.scene_rays(sc), sc["times"], AR.EDIT if edit else None)
    assert (~cand.any(-1)).sum() >= 1
    assert r["left_out"].mean() <= NR.LEFT_OUT_CAP
    assert np.isfinite(r["g"]).all() and np.isfinite(r["A"]).all() and (np.linalg.norm(r["g"], axis=-1) > 0).all()
    assert len(set(np.unique(r["hit"]))) == 4  # every actor wins somewhere, and some samples are outside


def test_the_edit_moves_the_boxes():
    base, moved = oracle_case("8x4_h32_sdf")[2], oracle_case("8x4_h32_sdf", edit=True)[2]
    assert (base["hit"] != moved["hit"]).sum() >= 5


# ---- the golden --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def golden_case(tag):
    p, ap = AR.field_params(8, 4, 32, tag == "sdf"), AR.actor_params(8, 4)
    return p, ap


@pytest.mark.parametrize("tag", ["sdf", "density"])
def test_restatement_agrees_with_the_reference_autograd(tag, gold):
    """gradient and geo of the reference's torch field with the scene's actors (fp32 autograd w.r.t. the sample positions),
    over the in-box samples and over the rest separately; the file holds no sample inside several boxes"""
    p, ap = golden_case(tag)
    r = AR.oracle_restatement(p, ap)
    rows = gold[f"{tag}_rows"]
    assert np.array_equal(rows, np.nonzero(r["n_boxes"] <= 1)[0]) and (r["n_boxes"] > 1).sum() > 0
    g, n, geo = (gold[f"{tag}_{k}"].astype(np.float64) for k in ("gradient", "normals", "geo"))
    inbox = r["hit"][rows] >= 0
    assert inbox.sum() >= 100 and (~inbox).sum() >= 100
    ex = (np.abs(g - r["g"][rows]) - NR.U * np.abs(r["g"][rows])) / (NR.U * np.maximum(r["A"][rows], 1e-300))
    for what, m in (("in-box", inbox), ("outside", ~inbox)):
        err = AR.rel_l2(g[m], r["g"][rows][m])
        print(f"{tag} {what}: rel-L2 {err:.3e}, largest excess {ex[m].max():.2f} units of 2^-24 A")
        assert err <= PARITY
        assert AR.rel_l2(geo[m], r["geo"][rows][m]) <= PARITY
        assert AR.rel_l2(n[m], r["normals"][rows][m]) <= PARITY
    unit = g / np.linalg.norm(g, axis=-1, keepdims=True)
    assert np.abs(n - (unit if tag == "sdf" else -unit)).max() < 1e-6


@pytest.mark.parametrize("variant", AR.VARIANTS)
def test_wrong_chains_are_told_apart(variant, gold):
    """rotating with W instead of W^T, no rotation, the static table's gradient kept for in-box samples, the static scale in
    the actor contraction: each misses the golden's in-box samples by far more than the parity bar"""
    p, ap = golden_case("sdf")
    r = AR.oracle_restatement(p, ap, variant=variant)
    rows = gold["sdf_rows"]
    inbox = r["hit"][rows] >= 0
    g = gold["sdf_gradient"].astype(np.float64)
    err = AR.rel_l2(g[inbox], r["g"][rows][inbox])
    print(f"{variant}: rel-L2 {err:.3e} on the in-box samples")
    assert err > 100 * PARITY
    if variant != "static_scale_in_the_actor_contraction":  # (that one changes the rows, hence the masks, everywhere)
        assert AR.rel_l2(g[~inbox], r["g"][rows][~inbox]) <= PARITY


def test_flip_enters_the_restatement():
    """diag(f, 1, 1): a flipped ray's in-box gradients differ from the unflipped ones, the others do not"""
    p, ap, base = oracle_case("8x4_h32_sdf")
    flipped = oracle_case("8x4_h32_sdf", flip=True)[2]
    f = np.repeat(AR.ray_flips(), AR.S)
    inbox = base["hit"] >= 0
    assert np.array_equal(base["hit"], flipped["hit"])
    same = (base["g"] == flipped["g"]).all(-1)
    assert same[~inbox].all() and same[inbox & (f > 0)].all() and not same[inbox & (f < 0)].any()


# ---- the entry points' host side ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(ge.LIB):
        ge.build()
    from neurad_studio_amd import _lib

    _lib.load()
    return _lib


def _field(lib, L=8, F=4, H=32, layers=2):
    one = 0x1000  # any non-null address: validation ends before anything is dereferenced
    f = lib.Field()
    f.grid.num_levels, f.grid.n_features, f.grid.log2_table_size, f.grid.param_dtype = L, F, 11, 0
    for i in range(L):
        f.grid.scalings[i] = 32.0 * (i + 1)
    f.table, f.static_scale, f.use_sdf = one, 100.0, 1
    f.geo.in_dim, f.geo.hidden_dim, f.geo.out_dim, f.geo.num_layers = L * F, H, 33, layers
    for k in range(layers):
        f.geo.weight[k] = f.geo.bias[k] = one
    return f


def _rays(lib, R, S, null=False):
    r = lib.Rays()
    r.n_rays, r.n_samples = R, S
    if not null:
        r.origins = r.directions = r.pixel_area = r.starts = r.ends = 0x1000
    return r


def _packed(lib, R, M, null=False):
    r = lib.PackedRays()
    r.n_rays, r.n_samples = R, M
    if not null:
        r.origins = r.directions = r.pixel_area = r.t_starts = r.t_ends = r.segments = 0x1000
    return r


def _actors(lib, L=4, F=4, dtype=0):
    one = 0x1000
    a = lib.Actors()
    a.n_times, a.n_actors, a.max_candidates = 5, 3, 3
    a.timestamps = a.positions = a.rotations_6d = a.present = a.bounds = a.tables = one
    a.grid.num_levels, a.grid.n_features, a.grid.log2_table_size, a.grid.param_dtype = L, F, 9, dtype
    for i in range(L):
        a.grid.scalings[i] = 64.0 * (i + 1)
    a.actor_scale = 10.0
    return a


def test_actor_entry_points_validate_on_the_host(lib):
    one = ctypes.c_void_p(0x1000)
    ref = ctypes.byref
    # (f, a, rays, cand x 3, flip, weights, [stride], geo, gradient, normals, ray_normals, hit, box_position)
    dense = lambda f, a, r, c, *outs: lib.call("nrhip_field_normals_actors", f, a, r, *c, None, None, 0, *outs, None)  # noqa: E731
    packed = lambda f, a, r, c, *outs: lib.call("nrhip_field_normals_packed_actors", f, a, r, *c, None, None, *outs, None)  # noqa: E731
    f, a, cand = _field(lib), _actors(lib), (one, one, one)
    grad_only = (None, one, None, None, None, None)
    rays = {dense: lambda R=4: ref(_rays(lib, R, 8, null=R == 0)), packed: lambda R=4: ref(_packed(lib, R, 8 if R else 0, null=R == 0))}
    for call in (dense, packed):
        call(ref(f), ref(a), rays[call](0), cand, *grad_only)  # R == 0: OK, no device pointer is read
        call(ref(f), ref(a), rays[call](0), cand, None, None, None, None, one, None)  # hit alone is an output
        with pytest.raises(lib.NeuradHipError, match="field descriptor is NULL"):
            call(None, ref(a), rays[call](), cand, *grad_only)
        with pytest.raises(lib.NeuradHipError, match="actors descriptor is NULL"):
            call(ref(f), None, rays[call](), cand, *grad_only)
        for k in range(3):
            with pytest.raises(lib.NeuradHipError, match="candidate list is NULL"):
                call(ref(f), ref(a), rays[call](), tuple(None if i == k else one for i in range(3)), *grad_only)
        with pytest.raises(lib.NeuradHipError, match="every output is NULL"):
            call(ref(f), ref(a), rays[call](), cand, None, None, None, None, None, None)
        with pytest.raises(lib.NeuradHipError, match="NULL"):
            call(ref(f), ref(a), None, cand, *grad_only)
        # shapes: the `Composite, Actors, F32` rows only -- (4, 8, 32) and (1, 4, 32) are static-only shapes
        for bad in (_field(lib, 4, 8, 32), _field(lib, 1, 4, 32), _field(lib, 8, 4, 48), _field(lib, 8, 4, 32, layers=3)):
            with pytest.raises(lib.NeuradHipError, match="code 2"):
                call(ref(bad), ref(a), rays[call](), cand, *grad_only)
        # the actor grid: the static grid's F and storage type, at most its levels
        for bad in (_actors(lib, 4, 2), _actors(lib, 4, 4, dtype=1), _actors(lib, 16, 4)):
            with pytest.raises(lib.NeuradHipError, match="code 2.*actor grid"):
                call(ref(f), ref(bad), rays[call](), cand, *grad_only)
    assert lib.normals_actors_c(4, 4, 32) == lib.normals_c(4, 4, 32) + 6


def test_header_states_the_actor_bound_constant():
    from host_gate import HEADER

    src = open(HEADER).read()
    assert "#define NRHIP_NORMALS_ACTORS_C(La, F, H) (NRHIP_NORMALS_C(La, F, H) + 6)" in src
    assert "nrhip_field_normals_actors" in src and "nrhip_field_normals_packed_actors" in src


def test_wrappers_check_the_actor_arguments(lib):
    import torch

    from neurad_studio_amd import ops

    z = torch.zeros
    spec = ops.GridSpec(8, 4, 11, 32, 8192)
    fs = ops.FieldSpec(spec, z(8 << 11, 4), 100.0, [z(32, 32), z(33, 32)], [z(32), z(33)], [z(32, 48), z(32, 32), z(32, 32)],
                       [z(32), z(32), z(32)])
    with pytest.raises(ValueError, match="ray_flip without actors"):
        ops.field_normals(fs, z(3, 3), z(3, 3), z(3), z(3, 5), z(3, 5), ray_flip=z(3))
    with pytest.raises(ValueError, match="want"):  # hit / box_position belong to the actor form
        ops.field_normals(fs, z(3, 3), z(3, 3), z(3), z(3, 5), z(3, 5), want=("hit",))
    with pytest.raises(NotImplementedError, match="box_position is the fused kernel's output"):  # up front, hits or none
        ops.field_normals_operators(fs, z(3, 3), z(3, 3), z(3), z(3, 5), z(3, 5), want=("box_position",), actors=(None, None))
    assert ops.normals_actors_c(4, 4, 32) == 4 + 4 + 32 + 246


def test_field_refuses_normals_with_actors_without_times_or_in_flipping_training():
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
    from neurad_studio_amd.model_components.dynamic_actors import DynamicActors, DynamicActorsConfig

    import builders

    cfg = NeuRADFieldConfig()
    cfg.grid.static.log2_hashmap_size = 8
    cfg.grid.actor.log2_hashmap_size = 8
    fld = NeuRADField(cfg, actors=DynamicActors(DynamicActorsConfig(), trajectories=builders.trajectories()), static_scale=100.0)
    fld.eval()
    assert fld.normals_fused()
    for what in ("compute_normals=True", "normals", "normals=True"):
        with pytest.raises(NotImplementedError, match=f"{what} with dynamic actors needs the rays' times"):
            fld._check_normals(what)
    fld._check_normals("normals", np.zeros(3))  # with times: covered
    fld.train()
    assert cfg.grid.actor.flip_prob > 0
    with pytest.raises(NotImplementedError, match="compute_normals=True with dynamic actors in training mode with actor.flip_prob"):
        fld._check_normals("compute_normals=True", np.zeros(3))
    cfg.grid.actor.flip_prob = 0.0
    fld._check_normals("compute_normals=True", np.zeros(3))
