"""Surface normals on the device (csrc/normals.hip: nrhip_field_normals / _packed; the contract and the error bound:
include/neurad_hip.h) against the numpy restatement of tests/normals_refs.py, which tests/test_normals_refs_host.py pins to
the reference's own autograd.  Per element |g_gpu - g| <= 2^-24 |g| + (c + 1) 2^-24 A with c = NRHIP_NORMALS_C(L, F, H), the
first-order rounding count stated in the header; a sample whose ReLU mask is decided within rounding is left out of the
element-wise comparison (at most 1 % of a case) and must still be finite."""
import functools

import numpy as np
import pytest
import torch

import builders
import normals_refs as NR
from gpu_util import bundle, cuda, dev, host, host64, make_actor_field, make_field, ops, small_model, to_spec  # noqa: F401

pytestmark = pytest.mark.gpu
ALL = ("geo", "gradient", "normals")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(oracle parameters, rays, restatement) of a case of normals_refs.CASES, computed once"""
    p, rays = NR.case_params(name)
    return p, rays, NR.restatement(p, *rays[:5])


@functools.lru_cache(maxsize=None)
def ragged():
    """six rays of up to 80 samples for the packed tests: (parameters, dense rays, restatement on all 6 x 80, counts)"""
    p = builders.field_params(True)
    rays = builders.sample_rays(6, 80, 11)
    return p, rays, NR.restatement(p, *rays[:5]), np.array([0, 1, 80, 17, 64, 5])


def rays_dev(rays):
    return tuple(dev(a) for a in rays[:5])


def check(out, r, p, rows=None, factor=1):
    """per-sample outputs (any leading shape) against the restatement's rows within ``factor`` times the bound"""
    c = NR.constant(p)
    sel = slice(None) if rows is None else rows
    keep = ~r["left_out"][sel]
    assert (~keep).mean() <= NR.LEFT_OUT_CAP
    g, A = r["g"][sel], r["A"][sel]
    if "gradient" in out:
        got = host64(out["gradient"]).reshape(-1, 3)
        assert np.isfinite(got).all()
        ex = (np.abs(got - g) - NR.U * np.abs(g)) / (NR.U * np.maximum(A, 1e-300))
        print(f"gradient: max excess {ex[keep].max():.2f} units of A, c = {c}")
        assert (np.abs(got - g) <= factor * NR.bound(g, A, c))[keep].all()
    if "normals" in out:
        got = host64(out["normals"]).reshape(-1, 3)
        assert np.isfinite(got).all()
        assert (np.abs(got - r["normals"][sel]) <= factor * NR.normal_tolerance(g, A, c))[keep].all()
        assert np.abs(np.linalg.norm(got, axis=-1) - 1).max() < 1e-6
    if "geo" in out:
        got = host64(out["geo"]).reshape(-1)
        assert np.isfinite(got).all()
        assert (np.abs(got - r["geo"][sel]) <= factor * NR.bound(r["geo"][sel], r["A_geo"][sel], c))[keep].all()


@pytest.mark.parametrize("name", list(NR.CASES))
def test_kernel_against_the_restatement(ops, name):
    p, rays, r = reference(name)
    L, F, H, use_sdf, R, S, half = NR.CASES[name]
    out = ops.field_normals(to_spec(ops, p, half), *rays_dev(rays), want=ALL)
    assert out["geo"].shape == (R, S) and out["gradient"].shape == (R, S, 3) and out["normals"].shape == (R, S, 3)
    check(out, r, p)
    if name == "neurad_density_h64":  # the density head's sign: against the gradient
        assert (host64(out["normals"]) * host64(out["gradient"])).sum(-1).max() < 0


def test_tie_rays_against_the_restatement(ops):
    """the rays of tests/golden/ray_grads_edges.npz: inf-norm ties, samples on the contraction's face, the rescale clamp at
    equality -- where torch picks one subgradient the kernel picks the same"""
    import os

    e = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_grads_edges.npz"))
    p = builders.field_params(True)
    p.static_scale = float(e["static_scale"])
    rays = tuple(e[k] for k in ("o", "d", "area", "starts", "ends"))
    r = NR.restatement(p, *rays)
    out = ops.field_normals(to_spec(ops, p), *rays_dev(rays), want=("gradient", "normals"))
    check(out, r, p)
    wrong = NR.restatement(p, *rays, ties="first", clamp_at_one=False)
    got = host64(out["gradient"]).reshape(-1, 3)
    miss = (np.abs(got - wrong["g"]) > NR.bound(r["g"], r["A"], NR.constant(p))).any(-1)
    assert miss.sum() >= 25  # the wrong subgradients are outside the bound on the tie samples


def test_bin_edges_in_place_and_a_permuted_order_give_the_same_bits(ops):
    p, rays, r = reference("neurad_sdf")
    fs = to_spec(ops, p)
    o, d, a, s, e = rays_dev(rays)
    base = ops.field_normals(fs, o, d, a, s, e, want=ALL)
    edges = dev(rays[5])  # [R, S + 1]: starts / ends as views, sample_stride = S + 1
    assert edges[:, :-1].stride(0) == s.shape[1] + 1
    view = ops.field_normals(fs, o, d, a, edges[:, :-1], edges[:, 1:], want=ALL)
    order = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(1)).to("cuda", torch.int32)
    perm = ops.field_normals(fs, o, d, a, s, e, want=ALL, order=order)
    for k in ALL:
        assert torch.equal(view[k], base[k]) and torch.equal(perm[k], base[k]), k


@pytest.mark.parametrize("name", ["neurad_sdf", "neurad_density_h64", "tiny_1x4"])
def test_geo_against_the_field_forward(ops, name):
    """geo sums the products of ops.field_fwd's sdf / raw output from the same encoding bits in another order (fma chains
    here, the matrix cores there): NOT to the bit, but within 2 (L F + H + 2) 2^-24 A_geo, the bound the header states"""
    p, rays, r = reference(name)
    L, F, H = NR.CASES[name][:3]
    fs = to_spec(ops, p)
    geo = host64(ops.field_normals(fs, *rays_dev(rays), want=("geo",))["geo"]).reshape(-1)
    fwd = host64(ops.field_fwd(fs, *rays_dev(rays))[1]).reshape(-1)
    assert (np.abs(geo - fwd) <= 2 * (L * F + H + 2) * NR.U * r["A_geo"]).all()


def test_weighted_ray_sum(ops):
    p, rays, r = reference("neurad_sdf")
    fs = to_spec(ops, p)
    o, d, a, s, e = rays_dev(rays)
    R, S = s.shape
    rng = np.random.default_rng(5)
    w = rng.random((R, S + 1)).astype(np.float32)
    w[rng.random((R, S + 1)) < 0.3] = 0
    w[3] = 0  # a ray of weight zero throughout
    wd = dev(w)[:, :S]  # a strided view: weight_stride = S + 1
    n = ops.field_normals(fs, o, d, a, s, e, want=("normals",))["normals"]
    out = ops.field_normals(fs, o, d, a, s, e, weights=wd)
    assert set(out) == {"gradient", "normals", "ray_normals"} and torch.equal(out["normals"], n)
    row = host(out["ray_normals"])
    assert row.shape == (R, 3) and (row[3] == 0).all()
    G, nh = NR.lanes_per_ray(S), host(n)
    for k in range(R):  # the kernel's own order, bit for bit, and the exactly rounded sum within the roundings
        assert np.array_equal(row[k], NR.ray_sum_sequential(w[k, :S], nh[k], G)), k
        exact, mag = NR.ray_sum_exact(w[k, :S], nh[k])
        assert (np.abs(row[k] - exact) <= (S + 8) * NR.U * mag).all()
    # a ray's row does not depend on its place in the batch, nor on the batch
    flip = torch.arange(R - 1, -1, -1, device="cuda")
    back = ops.field_normals(fs, o[flip], d[flip], a[flip], s[flip], e[flip], weights=wd[flip], want=("ray_normals",))
    assert torch.equal(back["ray_normals"][flip], out["ray_normals"])
    part = ops.field_normals(fs, o[11:18], d[11:18], a[11:18], s[11:18], e[11:18], weights=wd[11:18], want=("ray_normals",))
    assert torch.equal(part["ray_normals"], out["ray_normals"][11:18])
    # samples of weight zero are skipped: NaN intervals there leave every row as it was
    s2, e2 = s.clone(), e.clone()
    s2[wd == 0] = float("nan")
    e2[wd == 0] = float("nan")
    nan = ops.field_normals(fs, o, d, a, s2, e2, weights=wd, want=("ray_normals",))
    assert torch.equal(nan["ray_normals"], out["ray_normals"])


def packed_batch(rays, counts, order=None):
    """the first counts[r] samples of every ray, packed -> (t_starts, t_ends, segments, rows of the dense [R,S] batch)"""
    S = rays[3].shape[1]
    rows = np.concatenate([np.arange(c) + k * S for k, c in enumerate(counts)]).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dev(rays[3].reshape(-1)[rows]), dev(rays[4].reshape(-1)[rows]), cuda(seg), rows


def test_packed_samples(ops):
    """an empty segment, one of 1 sample, one of more than 64: per sample against the restatement and against the dense call on
    the same samples, per ray against the kernel's own order"""
    p, rays, r, counts = ragged()
    fs = to_spec(ops, p)
    o, d, a, s, e = rays_dev(rays)
    ts, te, seg, rows = packed_batch(rays, counts)
    M = rows.shape[0]
    w = np.random.default_rng(9).random(M).astype(np.float32)
    w[::5] = 0
    out = ops.field_normals_packed(fs, o, d, a, ts, te, seg, weights=dev(w), want=ALL + ("ray_normals",))
    assert out["geo"].shape == (M,) and out["gradient"].shape == (M, 3) and out["normals"].shape == (M, 3)
    check(out, r, p, rows)
    dense = ops.field_normals(fs, o, d, a, s, e, want=ALL)
    c = NR.constant(p)
    for k in ("gradient", "normals"):
        got, same = host64(out[k]), host64(dense[k]).reshape(-1, 3)[rows]
        tol = NR.bound(r["g"][rows], r["A"][rows], c) if k == "gradient" else NR.normal_tolerance(r["g"][rows], r["A"][rows], c)
        print(f"{k}: packed == dense bit for bit: {np.array_equal(got, same)}")
        assert (np.abs(got - same) <= tol).all()
    row, nh = host(out["ray_normals"]), host(out["normals"])
    G = NR.lanes_per_ray(-(-M // len(counts)))
    segs = np.concatenate([[0], np.cumsum(counts)])
    for k in range(len(counts)):
        assert np.array_equal(row[k], NR.ray_sum_sequential(w[segs[k]:segs[k + 1]], nh[segs[k]:segs[k + 1]], G)), k
    assert (row[0] == 0).all()  # the empty segment


def test_packed_without_samples_and_without_rays(ops):
    p, rays, r, counts = ragged()
    fs = to_spec(ops, p)
    o, d, a, s, e = rays_dev(rays)
    none = torch.empty(0, device="cuda")
    seg = torch.zeros(7, dtype=torch.int64, device="cuda")
    out = ops.field_normals_packed(fs, o, d, a, none, none, seg, weights=none, want=ALL + ("ray_normals",))  # M = 0
    assert out["gradient"].shape == (0, 3) and out["ray_normals"].shape == (6, 3) and not out["ray_normals"].any()
    out = ops.field_normals_packed(fs, o[:0], d[:0], a[:0], none, none, seg[:1], weights=none, want=ALL + ("ray_normals",))
    assert out["normals"].shape == (0, 3) and out["ray_normals"].shape == (0, 3)  # R = 0
    out = ops.field_normals(fs, o[:0], d[:0], a[:0], s[:0], e[:0], want=ALL)
    assert out["gradient"].shape == (0, 80, 3)


@pytest.mark.parametrize("name", ["neurad_sdf", "c2_sdf_h64", "neurad_density_h64"])
def test_operator_composition_agrees_within_twice_the_bound(ops, name):
    p, rays, r = reference(name)
    fs = to_spec(ops, p)
    R, S = rays[3].shape
    w = dev(np.random.default_rng(2).random((R, S)).astype(np.float32))
    fused = ops.field_normals(fs, *rays_dev(rays), weights=w, want=ALL + ("ray_normals",))
    oper = ops.field_normals_operators(fs, *rays_dev(rays), weights=w, want=ALL + ("ray_normals",))
    c = NR.constant(p)
    keep = ~r["left_out"]
    for k in ALL + ("ray_normals",):
        assert oper[k].shape == fused[k].shape, k
    dg = np.abs(host64(oper["gradient"]) - host64(fused["gradient"])).reshape(-1, 3)
    assert (dg <= 2 * NR.bound(r["g"], r["A"], c))[keep].all()
    dn = np.abs(host64(oper["normals"]) - host64(fused["normals"])).reshape(-1, 3)
    assert (dn <= 2 * NR.normal_tolerance(r["g"], r["A"], c))[keep].all()
    dgeo = np.abs(host64(oper["geo"]) - host64(fused["geo"])).reshape(-1)
    assert (dgeo <= 2 * NR.bound(r["geo"], r["A_geo"], c))[keep].all()
    check(oper, r, p)  # ... and is itself inside the bound
    # the per-ray sums: the per-sample tolerances weighted, plus the additions' own roundings (|n| <= 1)
    wh = host64(w)
    tol = (wh[..., None] * 2 * NR.normal_tolerance(r["g"], r["A"], c).reshape(R, S, 1)).sum(1) + (S + 8) * NR.U * wh.sum(-1)[:, None]
    if keep.all():
        assert (np.abs(host64(oper["ray_normals"]) - host64(fused["ray_normals"])) <= tol).all()


def field_samples(rays, packed=False):
    from neurad_studio_amd.cameras.rays import Frustums, RaySamples

    o, d, a, s, e = rays_dev(rays)
    R, S = s.shape
    per = lambda t, c: t.reshape(R, 1, c).expand(R, S, c)  # noqa: E731
    fr = dict(origins=per(o, 3), directions=per(d, 3), starts=s[..., None], ends=e[..., None], pixel_area=per(a, 1))
    if packed:
        fr = {k: v.reshape(R * S, -1).contiguous() for k, v in fr.items()}
    return RaySamples(frustums=Frustums(**fr))


@pytest.mark.parametrize("use_sdf", [True, False])
def test_field_forward_with_compute_normals(ops, use_sdf):
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as H

    fld = make_field(use_sdf).eval()
    p = builders.field_params(use_sdf)
    rays = builders.sample_rays(9, 13, 3)
    r = NR.restatement(p, *rays[:5])
    for packed in (False, True):
        rs = field_samples(rays, packed)
        with torch.no_grad():
            plain, out = fld(rs), fld(rs, compute_normals=True)
        assert set(out) == set(plain) | {H.NORMALS, H.GRADIENT}
        for k in plain:  # the other heads: bit for bit
            assert torch.equal(out[k], plain[k]), k
        shape = (9 * 13, 3) if packed else (9, 13, 3)
        assert out[H.NORMALS].shape == shape and out[H.GRADIENT].shape == shape
        check({"gradient": out[H.GRADIENT], "normals": out[H.NORMALS]}, r, p)
    out = fld(field_samples(rays), compute_normals=True)  # grad enabled: the two heads are detached all the same
    assert not out[H.NORMALS].requires_grad and not out[H.GRADIENT].requires_grad and out[H.FEATURE].requires_grad


def test_field_without_a_fused_shape_takes_the_operator_route(ops):
    """a hidden width the fused kernels are not instantiated for (H = 48): normals_fused() is False and the operator
    composition serves the two heads"""
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as H
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig

    cfg = NeuRADFieldConfig(geo_hidden_dim=48, nff_hidden_dim=48)
    cfg.grid.static.log2_hashmap_size = 11
    torch.manual_seed(0)
    fld = NeuRADField(cfg, actors=None, static_scale=100.0).cuda().eval()
    with torch.no_grad():
        fld.hashgrid.static_grid.hash_table.mul_(1000.0)
    assert not fld.normals_fused()
    rays = builders.sample_rays(5, 6, 3)
    with pytest.raises(Exception, match="code 2"):  # the fused entry point refuses the shape by name
        ops.field_normals(fld.field_spec(), *rays_dev(rays))
    with torch.no_grad():
        out = fld(field_samples(rays), compute_normals=True)
    g, n = out[H.GRADIENT], out[H.NORMALS]
    assert g.shape == (5, 6, 3) and torch.isfinite(g).all()
    assert torch.allclose(n, g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12), atol=1e-6)


def test_model_outputs_carry_the_normals():
    """normals=True on the fused eval route: NormalsRenderer of the per-sample normals and the non-sky weights (rel-L2 <= 1e-6,
    what the renderer's own test allows); every other output keeps its bits; the key is absent without the flag"""
    import synth
    from neurad_studio_amd.model_components.renderers import NormalsRenderer

    m = small_model(use_sdf=True).eval()
    R = 200
    o, d, area, _ = synth.rays(R, 21)

    def rays():
        return bundle(o, d, area / 9)

    with torch.no_grad():
        before = m.get_nff_outputs(rays())
    assert "normals" not in before
    seen = {}
    render = m.field.render

    def spy(o_, d_, area_, starts, ends, **kw):
        out = render(o_, d_, area_, starts, ends, **kw)
        seen.update(o=o_, d=d_, area=area_, starts=starts, ends=ends, out=out, kw=kw)
        return out

    m.field.render = spy
    m.normals = True
    with torch.no_grad():
        out = m.get_nff_outputs(rays())
    assert set(out) == set(before) | {"normals"} and seen["kw"]["return_weights"] is True
    for k in before:
        assert torch.equal(out[k], before[k]), k
    w, s, e = seen["out"][3][:, :-1], seen["starts"][:, :-1], seen["ends"][:, :-1]  # the non-sky samples
    per = m.field.normals(seen["o"], seen["d"], seen["area"], s, e, want=("normals",))["normals"]
    want = NormalsRenderer.forward(per, w.contiguous()[..., None])
    got = out["normals"]
    assert got.shape == (R, 3) and got.dtype == torch.float32
    rel = float((got.double() - want.double()).norm() / want.double().norm())
    print("model normals vs NormalsRenderer: rel-L2", rel)
    assert rel <= 1e-6
    lit = w.sum(-1) > 1e-3
    assert lit.any() and (got[lit].norm(dim=-1) - 1).abs().max() < 1e-5
    m.normals = False
    with torch.no_grad():
        assert set(m.get_nff_outputs(rays())) == set(before)


def test_dynamic_actors_are_refused_by_name():
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames as H  # noqa: F401

    fld = make_actor_field()
    rays = builders.sample_rays(4, 5, 3)
    with pytest.raises(NotImplementedError, match="compute_normals=True with dynamic actors"):
        fld(field_samples(rays), compute_normals=True)
    o, d, a, s, e = rays_dev(rays)
    with pytest.raises(NotImplementedError, match="with dynamic actors"):
        fld.normals(o, d, a, s, e)
    import synth

    m = small_model().eval()
    m.normals = True
    m.field.hashgrid.has_actors = lambda: True  # (the check comes first on the fused eval route: nothing else is reached)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="normals=True with dynamic actors"):
        m.fused_nff_outputs(bundle(*synth.rays(8, 21)[:3]))
