"""The fused render kernel on PACKED samples (nrhip_render_fwd_packed / ops.render_fwd_packed / NeuRADField.render_packed /
VolumetricSampler.render): one wavefront per ray over the ray's segment of the occupancy march's [M]-shaped intervals, the
field evaluated per 16-sample tile and composited as nrhip_packed_composite_fwd does (no sky-residual sample, depth over
all samples, zeros for a ray without samples).

References: (A) the numpy oracle's field, one sample per row with the ray's constants repeated, composited in float64 by
tests/packed_restatement.py -- bound TOL = 1e-4 rel-L2, the project's parity bound; (B) the route the packed samples took
before this kernel, ops.field_fwd on [M,1] + ops.packed_composite_fwd -- bound 1e-5, what test_render_fused_vs_oracle holds
fused vs unfused to."""
import functools

import numpy as np
import pytest
import torch

import neurad_oracle as O
import packed_restatement as PR
import synth
from conftest import rel_l2
from builders import field_params
from gpu_util import TOL, dev, host, make_field, ray_bundle, to_spec
from gpu_util import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

FUSED_GRIDS = ((16, 2), (8, 4), (4, 8), (1, 4), (4, 2), (4, 4), (8, 2))  # fields/neurad_field.py: _FUSED_GRIDS
# first / last ray empty, consecutive empties, exact multiples of 16, one long ray (carried scan), R not a multiple of 4
RAGGED = [0, 1, 15, 16, 17, 0, 0, 31, 32, 33, 48, 2, 64, 65, 130, 1, 0, 16, 16, 5, 250, 3, 0]
LG = 11  # T = 2^11 per level: seconds per test


def params(L, F, H, use_sdf, beta=3.0, scale=None):
    """field_params for any fused grid: geo layer 0 takes L * F inputs"""
    p = field_params(use_sdf=use_sdf, L=L, F=F, lg=LG, H=H, mn=16, mx=1024, scale=(2.0 if use_sdf else 0.5) if scale is None else scale)
    p.geo_b[0] = synth.linear(H, 32, 200)[1]  # this bias keeps the range of a 32-input layer whatever L * F is
    if use_sdf:
        p.beta = beta  # keeps alpha off saturation so that the compositing is exercised
    return p


@functools.lru_cache(maxsize=None)
def packed_rays(counts, seed):
    """-> o [R,3], d [R,3], area [R], t_starts [M], t_ends [M], seg [R+1]: sorted, contiguous intervals inside 0.1 .. 60 m"""
    counts = np.asarray(counts, np.int64)
    R = len(counts)
    o, d, area, _ = synth.rays(R, seed)
    rng = np.random.default_rng(seed)
    ts, te = [], []
    for n in counts:
        edges = np.sort(rng.uniform(0.1, 60.0, int(n) + 1)).astype(np.float32)
        ts.append(edges[:-1]), te.append(edges[1:])
    cat = lambda parts: np.concatenate(parts).astype(np.float32) if parts else np.zeros((0,), np.float32)  # noqa: E731
    return o, d, np.asarray(area, np.float32).reshape(-1), cat(ts), cat(te), PR.segments_from_counts(counts)


def oracle_route(p, rays):
    """(A): the oracle's field on M rays of one sample, composited in float64"""
    o, d, area, ts, te, seg = rays
    ri = PR.ray_indices_from_segments(seg)
    f = O.field_fwd(p, o[ri], d[ri], area[ri], ts[:, None], te[:, None])
    x = f["alpha"] if p.use_sdf else f["density"]
    feat, depth, acc, w = PR.composite(PR.f64(ts), PR.f64(te), PR.f64(x[:, 0]), PR.f64(f["feature"][:, 0]), seg, not p.use_sdf)
    return feat.numpy(), depth.numpy(), acc.numpy(), w.numpy()


def operator_route(ops, fs, rays):
    """(B): per-sample gathers + field_fwd [M,1] + packed_composite_fwd"""
    o, d, area, ts, te, seg = (dev(a) if a.dtype != np.int64 else dev(a, torch.int64) for a in rays)
    ri = dev(PR.ray_indices_from_segments(rays[5]), torch.int64)
    if ts.numel() == 0:
        z = lambda c: torch.zeros((o.shape[0], c), device="cuda")  # noqa: E731
        return z(32), z(1), z(1), ts
    feat, _, head = ops.field_fwd(fs, o[ri], d[ri], area[ri], ts[:, None], te[:, None])
    return ops.packed_composite_fwd(ts, te, head[:, 0], feat[:, 0], seg, not fs.use_sdf)


def fused_route(ops, fs, rays, **kw):
    o, d, area, ts, te, seg = (dev(a) if a.dtype != np.int64 else dev(a, torch.int64) for a in rays)
    return ops.render_fwd_packed(fs, o, d, area, ts, te, seg, return_weights=True, **kw)


def close(got, want, bound, what):
    for name, g, w in zip(("features", "depth", "accumulation", "weights"), got, want):
        g = host(g) if isinstance(g, torch.Tensor) else g
        w = host(w) if isinstance(w, torch.Tensor) else w
        err = rel_l2(g.reshape(-1), w.reshape(-1))
        print(f"{what} {name}: rel-L2 {err:.3e} (bound {bound:g})")
        assert err < bound or (name == "depth" and np.abs(g.reshape(-1) - w.reshape(-1)).max() < 1e-5), (what, name, err)


# ---- 1. ragged segments, every fused shape --------------------------------------------------------------------------
RAGGED_CASES = [(L, F, (32, 64)[(i + k) % 2], bool(k), False) for i, (L, F) in enumerate(FUSED_GRIDS) for k in (1, 0)] + \
    [(8, 4, 32, True, True)]


@pytest.mark.parametrize("L,F,H,use_sdf,half", RAGGED_CASES,
                         ids=[f"{L}x{F}-H{H}-{'sdf' if s else 'density'}{'-fp16' if h else ''}" for L, F, H, s, h in RAGGED_CASES])
def test_ragged_segments_every_fused_shape(ops, L, F, H, use_sdf, half):
    p = params(L, F, H, use_sdf)
    if half:
        p.grid.table = p.grid.table.astype(np.float16).astype(np.float32)  # the oracle sees the rounded table
    fs = to_spec(ops, p, half=half)
    rays = packed_rays(tuple(RAGGED), 7)
    got = fused_route(ops, fs, rays)
    assert got[0].shape == (23, 32) and got[1].shape == (23, 1) and got[2].shape == (23, 1) and got[3].shape == (sum(RAGGED),)
    close(got, oracle_route(p, rays), TOL, "vs oracle")
    close(got, operator_route(ops, fs, rays), 1e-5, "vs operator route")
    empty = torch.from_numpy(np.asarray(RAGGED) == 0).cuda()
    for t in got[:3]:  # a ray without samples: exactly zero, written by the kernel (the buffers come from torch.empty)
        assert bool((t[empty] == 0).all())
    # without the weights buffer: the same three per-ray outputs
    f2, d2, a2 = ops.render_fwd_packed(fs, *(dev(a) for a in rays[:5]), dev(rays[5], torch.int64))
    assert torch.equal(f2, got[0]) and torch.equal(d2, got[1]) and torch.equal(a2, got[2])


# ---- 2. a wave walks several rays -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L,F,H,use_sdf", [(8, 4, 32, True), (16, 2, 64, False)], ids=["8x4-H32-sdf", "16x2-H64-density"])
def test_a_wave_walks_many_rays_in_any_order(ops, L, F, H, use_sdf):
    """9001 rays are more than 4 x the persistent grid's waves (256 CUs x at most 4 workgroups x 4 waves = 4096 at the
    occupancy cap of the launch code; half of it at 2 workgroups per CU): every wave wraps from ray to ray many times, across
    empty rays too.  The processing order moves rays between waves and must not change a bit."""
    R = 9001
    counts = np.random.default_rng(17).integers(0, 41, R)
    assert (counts == 0).sum() >= 100 and (counts > 32).sum() >= 100
    rays = packed_rays(tuple(int(c) for c in counts), 19)
    fs = to_spec(ops, params(L, F, H, use_sdf))
    got = fused_route(ops, fs, rays)
    close(got, operator_route(ops, fs, rays), 1e-5, "vs operator route")
    order = dev(np.random.default_rng(23).permutation(R).astype(np.int32), torch.int32)
    perm = fused_route(ops, fs, rays, order=order)
    for a, b in zip(got, perm):
        assert torch.equal(a, b)
    empty = torch.from_numpy(counts == 0).cuda()
    assert bool((got[0][empty] == 0).all()) and bool((got[2][empty] == 0).all())


# ---- 3. degenerate batches ------------------------------------------------------------------------------------------
def test_degenerate_batches(ops):
    p = params(8, 4, 32, True)
    fs = to_spec(ops, p)
    # R = 5, M = 0: zeros, no sample pointer exists at all
    f, d, a, w = fused_route(ops, fs, packed_rays((0, 0, 0, 0, 0), 3))
    assert f.shape == (5, 32) and w.shape == (0,)
    assert bool((f == 0).all()) and bool((d == 0).all()) and bool((a == 0).all())
    # R = 0: a no-op
    z = lambda *s: torch.zeros(s, device="cuda")  # noqa: E731
    f, d, a, w = ops.render_fwd_packed(fs, z(0, 3), z(0, 3), z(0), z(0), z(0), torch.zeros(1, dtype=torch.int64, device="cuda"),
                                       return_weights=True)
    assert f.shape == (0, 32) and d.shape == (0, 1) and a.shape == (0, 1) and w.shape == (0,)
    for counts in ((1,), (1000,)):
        rays = packed_rays(counts, 5)
        got = fused_route(ops, fs, rays)
        close(got, oracle_route(p, rays), TOL, f"n = {counts[0]} vs oracle")
        close(got, operator_route(ops, fs, rays), 1e-5, f"n = {counts[0]} vs operator route")
    from neurad_studio_amd._lib import NeuradHipError

    rays = packed_rays((3, 4), 5)
    with pytest.raises(NeuradHipError):
        fused_route(ops, fs, rays, early_stop_eps=1.5)
    with pytest.raises(ValueError):  # per-ray tensors must have R = len(segments) - 1 rows
        ops.render_fwd_packed(fs, z(3, 3), z(3, 3), z(3), dev(rays[3]), dev(rays[4]), dev(rays[5], torch.int64))


# ---- 4. uniform segments against the dense kernel --------------------------------------------------------------------
@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
def test_uniform_segments_against_the_dense_kernel(ops, use_sdf):
    """Every segment 32 samples long: the dense kernel's arithmetic with another addressing.  Its features carry the sky
    residual (1 - acc) x the last sample's feature and its depth leaves the last sample out; both are removed with the
    per-sample kernel's last-sample feature."""
    R, S = 33, 32
    rays = packed_rays((S,) * R, 29)
    o, d, area, ts, te, seg = rays
    fs = to_spec(ops, params(8, 4, 32, use_sdf))
    got = fused_route(ops, fs, rays)
    st, en = dev(ts.reshape(R, S)), dev(te.reshape(R, S))
    df, dd, da, dw = ops.render_fwd(fs, dev(o), dev(d), dev(area), st, en, return_weights=True)
    assert rel_l2(host(got[3]), host(dw).reshape(-1)) < 1e-6 and rel_l2(host(got[2]), host(da)) < 1e-6
    print("weights bitwise equal:", torch.equal(got[3], dw.reshape(-1)), " accumulation:", torch.equal(got[2], da))
    feat = ops.field_fwd(fs, dev(o), dev(d), dev(area), st, en)[0]  # [R,S,32]
    want_f = df - (1.0 - da) * feat[:, -1]
    want_d = dd + dw[:, -1:] * (st[:, -1:] + en[:, -1:]) / 2
    assert rel_l2(host(got[0]), host(want_f)) < 1e-5 and rel_l2(host(got[1]), host(want_d)) < 1e-5


# ---- 5. pair products --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,F,H", [(16, 2, 64), (8, 4, 32)], ids=["16x2-H64", "8x4-H32"])
def test_pair_products_are_fp32_equivalent(ops, switches, L, F, H):
    rays = packed_rays(tuple(RAGGED), 7)

    def both(fs):
        switches.set("NRHIP_MLP_PAIRS", "0")
        a = fused_route(ops, fs, rays)
        switches.unset("NRHIP_MLP_PAIRS")  # the default: fp16 pairs
        b = fused_route(ops, fs, rays)
        return a, b

    f32, prs = both(to_spec(ops, params(L, F, H, True)))
    close(prs, f32, 1e-6, "pairs vs fp32 products")
    assert not torch.equal(prs[0], f32[0])  # (a different kernel did run)
    # activations beyond the pair's range in some tiles (|x| >= 1000): those tiles take the fp32 products
    big = params(L, F, H, True)
    big.grid.table[::2] *= 3.0e3
    f32, prs = both(to_spec(ops, big))
    assert all(bool(torch.isfinite(t).all()) for t in prs)
    close(prs, f32, 1e-5, "pairs vs fp32 products, fp32 escape")


# ---- 6. early termination ------------------------------------------------------------------------------------------------
def test_early_termination_is_bounded_and_tile_granular(ops):
    eps = 1e-3
    counts = tuple([96, 40, 130, 7, 0, 64, 33, 16] * 8)
    rays = packed_rays(counts, 31)
    seg = rays[5]
    fs = to_spec(ops, params(8, 4, 32, True, beta=6.0))  # alphas around 0.5: the transmittance is below 1e-3 after a dozen samples
    f0, d0, a0, w0 = fused_route(ops, fs, rays)
    f1, d1, a1, w1 = fused_route(ops, fs, rays, early_stop_eps=eps)
    w0h, w1h = host(w0).astype(np.float64), host(w1)
    skipped = np.zeros(w0h.shape[0], bool)
    for r in range(len(counts)):  # the kernel's rule: the tile whose ENTERING transmittance is below eps is the ray's last
        b, e = int(seg[r]), int(seg[r + 1])
        for k in range(1, (e - b + 15) // 16):
            if 1.0 - w0h[b:b + 16 * k].sum() < eps * 0.5:  # (margin: the fp32 carry against this float64 sum)
                skipped[b + 16 * (k + 1):e] = True
                break
    assert skipped.mean() > 0.25, "the scene must terminate rays early"
    assert (w1h[skipped] == 0).all()
    kept = ~((w1h == 0) & (w0h != 0))
    assert np.array_equal(w1h[kept], host(w0)[kept])  # in front of the cut: the same bits
    assert float((a1 - a0).abs().max()) < eps
    assert float((f1 - f0).abs().max()) <= 3 * eps * float(f0.abs().max())
    for a, b in zip(fused_route(ops, fs, rays, early_stop_eps=0.0), (f0, d0, a0, w0)):
        assert torch.equal(a, b)


# ---- 7. module level -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_sdf", [True, False], ids=["sdf", "density"])
def test_volumetric_sampler_render(ops, use_sdf, monkeypatch):
    from neurad_studio_amd.field_components.field_heads import FieldHeadNames
    from neurad_studio_amd.fields.neurad_field import NeuRADField, NeuRADFieldConfig
    from neurad_studio_amd.model_components.ray_samplers import VolumetricSampler
    from neurad_studio_amd.model_components.renderers import render_packed
    from neurad_studio_amd.shims.nerfacc import OccGridEstimator

    R = 96
    est = OccGridEstimator([-5, -5, -5, 5, 5, 5], resolution=16)
    est.binaries[0] = dev(np.random.default_rng(3).random((16, 16, 16)) < 0.3)
    rb = ray_bundle(R, 90, far=9.0)
    sampler = VolumetricSampler(est).eval()
    kw = dict(render_step_size=0.1, cone_angle=0.0)
    fld = make_field(use_sdf).eval()
    assert fld.fused_packed_supported()
    # the route the samples took before: gathers -> field [M,1] -> packed compositing
    with torch.no_grad():
        rs, ri = sampler(rb, **kw)
        out = fld(rs)
        head = {"alpha": out[FieldHeadNames.ALPHA]} if use_sdf else {"density": out[FieldHeadNames.DENSITY]}
        want = render_packed(out[FieldHeadNames.FEATURE], rs, ri, R, **head)
    counts = torch.bincount(ri, minlength=R).cpu().numpy()
    assert ri.shape[0] > 1000 and (counts == 0).sum() >= 4 and counts.max() >= 33
    # the fused route reads the bundle's own tensors: no per-sample field evaluation, no gather of the ray constants
    with monkeypatch.context() as m:
        def refuse(*a, **k):
            raise AssertionError("the fused route must not go through the per-sample field kernel")
        m.setattr(ops, "field_fwd", refuse)
        m.setattr(VolumetricSampler, "_gather", staticmethod(refuse))
        got = sampler.render(fld, rb, **kw)
    assert set(got) == {"features", "depth", "accumulation", "weights", "ray_indices", "t_starts", "t_ends"}
    assert torch.equal(got["ray_indices"], ri) and got["weights"].shape == (ri.shape[0], 1)
    assert torch.equal(got["t_starts"], rs.frustums.starts[:, 0]) and torch.equal(got["t_ends"], rs.frustums.ends[:, 0])
    for key in ("features", "depth", "accumulation", "weights"):
        err = rel_l2(host(got[key]), host(want[key]))
        print(f"{key}: rel-L2 {err:.3e}")
        assert err < 1e-5, key
    # a field outside the gate: the same keys through forward() + renderers.render_packed
    cfg = NeuRADFieldConfig(use_sdf=use_sdf)
    cfg.grid.static.log2_hashmap_size, cfg.grid.static.num_levels = LG, 3
    torch.manual_seed(4)
    odd = NeuRADField(cfg, actors=None, static_scale=100.0).cuda().eval()
    assert not odd.fused_packed_supported()
    fb = sampler.render(odd, rb, **kw)
    assert set(fb) == set(got) and torch.equal(fb["ray_indices"], ri) and fb["features"].shape == (R, 32)
    assert fb["weights"].shape == (ri.shape[0], 1) and bool(torch.isfinite(fb["features"]).all())
    with pytest.raises(NotImplementedError, match="operator path"):
        with torch.no_grad():
            odd.render_packed(rb.origins, rb.directions, rb.pixel_area, got["t_starts"], got["t_ends"], ray_indices=ri, num_rays=R)
    # a march without samples: zero rows, from either route
    far_away = ray_bundle(8, 91, far=9.0)
    far_away.origins[:] = torch.tensor([50.0, 50.0, 50.0], device="cuda")
    far_away.directions[:] = torch.tensor([1.0, 0.0, 0.0], device="cuda")
    for f_ in (fld, odd):
        none = sampler.render(f_, far_away, **kw)
        assert none["weights"].shape == (0, 1) and none["features"].shape == (8, 32)
        assert all(bool((none[k] == 0).all()) for k in ("features", "depth", "accumulation"))
    with pytest.raises(RuntimeError, match="eval"):
        VolumetricSampler(est).train().render(fld, rb, **kw)


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_bitwise(ops):
    fs = to_spec(ops, params(8, 4, 32, True))
    rays = packed_rays(tuple(RAGGED), 7)
    o, d, area, ts, te = (dev(a) for a in rays[:5])
    seg = dev(rays[5], torch.int64)
    eager = ops.render_fwd_packed(fs, o, d, area, ts, te, seg, return_weights=True)
    torch.cuda.synchronize()  # (the eager call has also made the kernel's one-time occupancy query)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.render_fwd_packed(fs, o, d, area, ts, te, seg, return_weights=True)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)


# ---- 9. a preferred row without a packed form --------------------------------------------------------------------------
FALLBACK_COUNTS = (0, 1, 15, 16, 17, 33, 0)
FALLBACK_LG = 15  # level 0 (resolution 16) gets a shadow copy in the eval table: 3 * 5 bits <= log2 T


def fallback_setup(ops, H, half):
    p = field_params(use_sdf=True, L=8, F=4, lg=FALLBACK_LG, H=H, mn=16, mx=1024, scale=2.0)
    p.beta = 3.0
    rays = packed_rays(FALLBACK_COUNTS, 37)
    assert rays[3].shape[0] == sum(FALLBACK_COUNTS) == 82
    return to_spec(ops, p, half=half), rays


# (8, 4, 32): no split row, the switch changes nothing on the dense side either | (8, 4, 64): choose_variant prefers the
# `Composite, Static, Bf16Split` row, which has no packed form
@pytest.mark.parametrize("H", [32, 64], ids=["H32", "H64"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_packed_render_falls_back_from_the_split_products(ops, switches, H, half):
    fs, rays = fallback_setup(ops, H, half)
    switches.set("NRHIP_MLP_PAIRS", "0")
    want = fused_route(ops, fs, rays)
    switches.set("NRHIP_MLP_SPLIT_BF16", "1")
    got = fused_route(ops, fs, rays)
    assert len(got) == 4
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_packed_training_forward_falls_back_from_the_pair_products(ops, switches, half):
    """NRHIP_MLP_PAIRS_TRAIN=1 makes the `PerSample, Static, F16Pairs` row the preferred one; packed rows exist with fp32
    products only"""
    fs, rays = fallback_setup(ops, 32, half)
    args = [dev(a) for a in rays[:5]] + [dev(rays[5], torch.int64)]
    want = ops.field_fwd_train_packed(fs, *args)
    switches.set("NRHIP_MLP_PAIRS_TRAIN", "1")
    got = ops.field_fwd_train_packed(fs, *args)
    buffers = lambda res: list(res[0]) + list(res[1])  # noqa: E731
    assert len(buffers(got)) == 7
    for a, b in zip(buffers(got), buffers(want)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_packed_render_ignores_a_handed_over_eval_table(ops, switches, monkeypatch, half):
    """A field descriptor with eval_table / eval_layout makes the eval-table row the preferred one; it has no packed form,
    and the fp32 row that runs instead reads the plain table."""
    from neurad_studio_amd import _lib

    fs, rays = fallback_setup(ops, 32, half)
    switches.set("NRHIP_MLP_PAIRS", "0")
    monkeypatch.setattr(ops, "_EVAL_RELAYOUT", True)
    ops.clear_eval_tables()
    relaid = ops.eval_table(fs.grid, fs.table)
    assert relaid is not None
    r, keep = ops._c_packed_rays("render_fwd_packed", *(dev(a) for a in rays[:5]), dev(rays[5], torch.int64))

    def run(with_eval_table):
        f, keep2 = fs.c_field()
        if with_eval_table:
            f.eval_table, f.eval_layout = relaid[0].data_ptr(), relaid[1]
        out = [torch.empty((7, 32), device="cuda"), torch.empty((7, 1), device="cuda"), torch.empty((7, 1), device="cuda"),
               torch.empty((82,), device="cuda")]
        _lib.call("nrhip_render_fwd_packed", f, r, *(ops._ptr(t) for t in out), 0.0, ops._stream())
        torch.cuda.synchronize()
        return out

    want, got = run(False), run(True)
    ops.clear_eval_tables()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert bool((want[2][1:6] > 0).all())  # (the rays with samples did render something)
