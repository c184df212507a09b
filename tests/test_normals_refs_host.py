"""CPU checks of the surface normals (csrc/normals.hip; the contract: include/neurad_hip.h at nrhip_field_normals): the
numpy restatement of tests/normals_refs.py against the reference's own autograd (tests/golden/normals.npz, made by
scripts/make_golden_normals.py) -- which pins the sign, the chain and the tie rules -- the share of samples the GPU tests may
leave out, and the host-side argument checks of the two entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

import builders
import normals_refs as NR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "normals.npz"))


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(GOLD, "ray_grads_edges.npz"))


def golden_case(tag, gold, edges):
    if tag == "edges":
        p = builders.field_params(True)
        p.static_scale = float(edges["static_scale"])
        return p, tuple(edges[k] for k in ("o", "d", "area", "starts", "ends"))
    return builders.field_params(tag == "sdf"), builders.sample_rays(*(int(v) for v in gold["rays"]))[:5]


@pytest.mark.parametrize("tag", ["sdf", "density", "edges"])
def test_restatement_agrees_with_the_reference_autograd(tag, gold, edges):
    """gradient, normal and geo of the reference's torch field (fp32 autograd w.r.t. the sample positions) within the bound
    the kernel is held to: sign, chain and subgradients are the reference's"""
    p, rays = golden_case(tag, gold, edges)
    r = NR.restatement(p, *rays)
    c = NR.constant(p)
    g, n, geo = (gold[f"{tag}_{k}"].astype(np.float64) for k in ("gradient", "normals", "geo"))
    assert g.shape == r["g"].shape and not r["left_out"].any()
    assert (np.abs(g - r["g"]) <= NR.bound(r["g"], r["A"], c)).all()
    assert (np.abs(n - r["normals"]) <= NR.normal_tolerance(r["g"], r["A"], c)).all()
    assert (np.abs(geo - r["geo"]) <= NR.bound(r["geo"], r["A_geo"], c)).all()
    # the sign, said once more without the restatement: an SDF's normal is the normalised gradient, the density's its negative
    unit = g / np.linalg.norm(g, axis=-1, keepdims=True)
    assert np.abs(n - (unit if tag != "density" else -unit)).max() < 1e-6
    assert (np.linalg.norm(g, axis=-1) > 0).all()


def test_wrong_subgradients_are_told_apart_on_the_tie_rays(gold, edges):
    """ties="first" (the whole inf-norm gradient to the first maximal axis) and no clamp gradient at equality miss the
    reference by more than the bound on tie rays, and only there"""
    p, rays = golden_case("edges", gold, edges)
    S = edges["starts"].shape[1]
    kind = np.repeat(edges["kind"], S)
    g = gold["edges_gradient"].astype(np.float64)
    c = NR.constant(p)
    good, bad = NR.restatement(p, *rays), NR.restatement(p, *rays, ties="first", clamp_at_one=False)
    miss = (np.abs(g - bad["g"]) > NR.bound(good["g"], good["A"], c)).any(-1)
    assert not (np.abs(g - good["g"]) > NR.bound(good["g"], good["A"], c)).any()
    assert miss[kind == 1].sum() >= 20 and miss[kind == 3].sum() >= 5  # inf-norm ties; the rescale clamp at equality
    assert not miss[kind == 0].any()


@pytest.mark.parametrize("name", list(NR.CASES))
def test_left_out_share_of_the_gpu_cases(name):
    """at most 1 % of a case's samples have a hidden pre-activation within rounding of zero; none has a zero gradient"""
    p, rays = NR.case_params(name)
    r = NR.restatement(p, *rays[:5])
    assert r["left_out"].mean() <= NR.LEFT_OUT_CAP
    assert (np.linalg.norm(r["g"], axis=-1) > 0).all() and np.isfinite(r["g"]).all() and np.isfinite(r["A"]).all()


def test_ray_sum_restatement_orders():
    """the sequential fp32 order of a group of G lanes against the exactly rounded sum: they agree within the products' roundings
    and the additions', and a sample of weight zero holding a NaN normal changes neither"""
    rng = np.random.default_rng(3)
    w = rng.random(70).astype(np.float32)
    n = rng.standard_normal((70, 3)).astype(np.float32)
    w[5] = 0
    n[5] = np.nan
    for G in (1, 16, 64):
        seq = NR.ray_sum_sequential(w, n, G)
        exact, mag = NR.ray_sum_exact(w, n)
        assert np.isfinite(seq).all() and (np.abs(seq - exact) <= (70 + 8) * NR.U * mag).all()
    assert [NR.lanes_per_ray(s) for s in (0, 1, 2, 3, 16, 17, 64, 65, 1000)] == [1, 1, 2, 4, 16, 32, 64, 64, 64]


# ---- the entry points' host side ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(ge.LIB):
        ge.build()
    from neurad_studio_amd import _lib

    _lib.load()
    return _lib


def _field(lib, L=8, F=4, H=32, layers=2, bias=True):
    one = 0x1000  # any non-null address: validation ends before anything is dereferenced
    f = lib.Field()
    f.grid.num_levels, f.grid.n_features, f.grid.log2_table_size, f.grid.param_dtype = L, F, 11, 0
    for i in range(L):
        f.grid.scalings[i] = 32.0 * (i + 1)
    f.table, f.static_scale, f.use_sdf = one, 100.0, 1
    f.geo.in_dim, f.geo.hidden_dim, f.geo.out_dim, f.geo.num_layers = L * F, H, 33, layers
    for k in range(layers):
        f.geo.weight[k] = one
        f.geo.bias[k] = one if bias else None
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


def test_entry_points_validate_on_the_host(lib):
    one = ctypes.c_void_p(0x1000)
    ref = ctypes.byref
    dense = lambda f, r, w, ws, *outs: lib.call("nrhip_field_normals", f, r, w, ws, *outs, None)  # noqa: E731
    packed = lambda f, r, w, *outs: lib.call("nrhip_field_normals_packed", f, r, w, *outs, None)  # noqa: E731
    f = _field(lib)
    # no-ops that read no device pointer: no rays (every ray pointer NULL)
    dense(ref(f), ref(_rays(lib, 0, 8, null=True)), None, 0, None, one, None, None)
    packed(ref(f), ref(_packed(lib, 0, 0, null=True)), None, None, None, one, None)
    with pytest.raises(lib.NeuradHipError, match="field descriptor is NULL"):
        dense(None, ref(_rays(lib, 4, 8)), None, 0, None, one, None, None)
    with pytest.raises(lib.NeuradHipError, match="field descriptor is NULL"):
        packed(None, ref(_packed(lib, 4, 8)), None, None, one, None, None)
    with pytest.raises(lib.NeuradHipError, match="NULL"):
        dense(ref(f), None, None, 0, None, one, None, None)
    with pytest.raises(lib.NeuradHipError, match="NULL"):
        packed(ref(f), None, None, None, one, None, None)
    with pytest.raises(lib.NeuradHipError, match="every output is NULL"):
        dense(ref(f), ref(_rays(lib, 4, 8)), None, 0, None, None, None, None)
    with pytest.raises(lib.NeuradHipError, match="every output is NULL"):
        packed(ref(f), ref(_packed(lib, 4, 8)), None, None, None, None, None)
    with pytest.raises(lib.NeuradHipError, match="ray_normals without weights"):
        dense(ref(f), ref(_rays(lib, 4, 8)), None, 0, None, None, None, one)
    with pytest.raises(lib.NeuradHipError, match="ray_normals without weights"):
        packed(ref(f), ref(_packed(lib, 4, 8)), None, None, None, None, one)
    with pytest.raises(lib.NeuradHipError, match="weight_stride"):
        dense(ref(f), ref(_rays(lib, 4, 8)), one, 7, None, None, None, one)
    with pytest.raises(lib.NeuradHipError, match="NULL pointer"):  # rays to read, none given
        dense(ref(f), ref(_rays(lib, 4, 8, null=True)), None, 0, None, one, None, None)
    with pytest.raises(lib.NeuradHipError, match="NULL pointer"):
        packed(ref(f), ref(_packed(lib, 4, 8, null=True)), None, None, one, None, None)
    with pytest.raises(lib.NeuradHipError, match="samples without rays"):
        packed(ref(f), ref(_packed(lib, 0, 8)), None, None, one, None, None)
    with pytest.raises(lib.NeuradHipError, match=r"code 2.*2\^31"):
        packed(ref(f), ref(_packed(lib, 4, 1 << 31)), None, None, one, None, None)
    # shapes: only the `PerSample, Static, F32` rows with a two-layer geometry MLP that has its biases
    for bad in (_field(lib, 2, 4), _field(lib, 8, 4, 48), _field(lib, 8, 4, 32, layers=3), _field(lib, 8, 4, bias=False)):
        with pytest.raises(lib.NeuradHipError, match="code 2"):
            dense(ref(bad), ref(_rays(lib, 4, 8)), None, 0, None, one, None, None)
        with pytest.raises(lib.NeuradHipError, match="code 2"):
            packed(ref(bad), ref(_packed(lib, 4, 8)), None, None, one, None, None)
    assert lib.normals_c(8, 4, 32) == 8 + 4 + 32 + 240


def test_header_states_the_bound_constant():
    from host_gate import HEADER

    src = open(HEADER).read()
    assert "#define NRHIP_NORMALS_C(L, F, H) ((H) + (L) + (F) + 240)" in src


def test_wrappers_refuse_cpu_tensors_and_bad_arguments(lib):
    from neurad_studio_amd import ops

    z = torch.zeros
    spec = ops.GridSpec(8, 4, 11, 32, 8192)
    fs = ops.FieldSpec(spec, z(8 << 11, 4), 100.0, [z(32, 32), z(33, 32)], [z(32), z(33)], [z(32, 48), z(32, 32), z(32, 32)],
                       [z(32), z(32), z(32)])
    for fn in (ops.field_normals, ops.field_normals_operators):
        with pytest.raises(lib.NeuradHipError):  # CPU tensors: refused, not computed on the host
            fn(fs, z(3, 3), z(3, 3), z(3), z(3, 5), z(3, 5))
        with pytest.raises(ValueError, match="ray_normals needs weights"):
            fn(fs, z(3, 3), z(3, 3), z(3), z(3, 5), z(3, 5), want=("ray_normals",))
        with pytest.raises(ValueError, match="want"):
            fn(fs, z(3, 3), z(3, 3), z(3), z(3, 5), z(3, 5), want=("depth",))
    with pytest.raises(lib.NeuradHipError):
        ops.field_normals_packed(fs, z(3, 3), z(3, 3), z(3), z(7), z(7), z(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="ray_normals needs weights"):
        ops.field_normals_packed(fs, z(3, 3), z(3, 3), z(3), z(7), z(7), z(4, dtype=torch.int64), want=("ray_normals",))


def test_field_refuses_multisamples_by_name():
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig

    cfg = NeuRADFieldConfig(num_multisamples=3)
    cfg.grid.static.log2_hashmap_size = 8
    fld = NeuRADField(cfg, actors=None, static_scale=100.0)
    with pytest.raises(NotImplementedError, match="num_multisamples"):
        fld._check_normals("compute_normals=True")
    assert not fld.normals_fused()
